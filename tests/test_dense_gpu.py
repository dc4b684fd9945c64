"""The dense-layer and fused-MLP kernels alone, against float64 at the shapes where their launchers change kernel.

Kernels: dense_fwd / dense_fwd_splitk / dense_dgrad / dense_wgrad (csrc/backbone.hip) and mlp_tail_fwd /
mlp_tail_bwd / mlp_transpose / rows_wgrad (csrc/mlp.hip), through the thin entry points of csrc/ops_api.hip.

Reference and bound.  The reference is float64 torch on the CPU of the same operation on the same fp32 inputs.  The
bound is per element, |out - ref| <= 1e-5 * mag, with mag the same operation on absolute values (sum |a||b| + |bias|,
times the dropout / gate scale where one applies): the project's fp32-accumulation level.  It is not tuned to the
kernels; every test prints its worst err / mag (run with -s), recorded below.  Outputs are prefilled with NaN and must
be finite afterwards (so is every scratch buffer: an unwritten split-K slab would show), a sentinel behind every scratch
and rows_wgrad output must survive, and where a device flag says "do not run" the sentinel prefill must be unchanged.

Decisions.  Dropout is exact: where oracle.rng.dropout_keep says dropped the output is 0.0, and the non-zero pattern
equals keep & (z > 0).  A ReLU decision within rounding of zero may go either way: elements whose float64
pre-activation has |z| <= 1e-5 * mag are left out, at most 1 in 1000 per checked tensor (the host-only test below shows
the float64 reference alone stays under that at these seeds).  The gates of the input gradients (dense_dgrad's gate,
the chain's h[i]) are inputs, so `gate > 0` is exact and nothing is excluded there.  The MLP chain is checked layer by
layer, each against the float64 layer applied to the device's own previous output, so a rounding-level flip cannot
cascade.

Branch boundaries (read from the launchers; BK = 32, 64x64 MFMA tiles):
  dense_fwd    skinny<8> M <= 8, skinny<16> M <= 16, both only when K % 4 == 0; a thread's second unrolled step at
               K/4 > 512, a second trip of its outer loop at K/4 > 2048; otherwise MFMA with
               splits = min(ceil(256 / tiles), ceil(K / 128)), capped by max_splits and halved until they fit the scratch.
  dense_dgrad  skinny when M <= 16, N % 4 == 0 and (N + 512) * (M <= 8 ? 8 : 16) * 4 <= 65536 (N <= 1536 / N <= 512);
               otherwise MFMA, split-K only with a scratch, tiles < 64 and N >= 256 (splits = min(256 / tiles, N / 128)).
  dense_wgrad  skinny when M <= 16 and K % 4 == 0 (a second block in x at K/4 > 256); otherwise MFMA over GN = K + 1
               columns (the bias as a ones column), splits = min(ceil(target_blocks / tiles), ceil(M / 128)).
  mlp_tail_fwd rows per block 2 / 4 / 8 (auto: 4 at M >= 64, else 8); 1024 threads with mlp_tail_wide except at 8
               rows, which always runs 256 threads.  The K0 = 96 and 40 chains give dense_fwd_splitk one slab; the
               K0 = 520 chain (added here) gives five, which crosses the 4-slab load batch of the tail's layer-0 sum.

Bit-identity across rows per block.  Rows are independent in mlp_tail_fwd_kernel and the K-slice count
P = min(NTH / (N/4), K/8) does not depend on the rows per block, but it does depend on the thread count NTH, and the
launcher has no 1024-thread instance for 8 rows: with mlp_tail_wide = 1, rb = 8 runs <8, 256> while rb = 2 and 4 run
<.., 1024>, so their K-slices differ and the sums round differently.  That is no leak between rows.  What the code
promises, and the test asserts, is: all five outputs bit-identical across rb in {2, 4, 8} with mlp_tail_wide = 0,
across rb in {2, 4} with mlp_tail_wide = 1, rb = 8 the same under either setting, and rb = 0 the same as the rb it picks.

mlp_tail_bwd at widths that are no multiple of 4 (24, 10, 6, 7, 3): the kernel now zeroes the pad columns of each
ping-pong buffer.  The case must come out finite and within the bound; a pass cannot prove the old code wrong, since
what stale LDS holds is not controllable (and nothing is done to provoke it).

Measured on an MI355X, one run of this file (worst err / mag per branch, against the bound of 1e-5; excluded
elements are 0 everywhere except where a share is given):
  dense_fwd    skinny<8> 2.2e-8, skinny<16> 4.0e-8, MFMA one split 1.8e-7, MFMA split-K 3.9e-8 (8 slabs), 7.4e-8
               (halved to 2, and max_splits = 2), 1.4e-7 (no scratch: one split); with relu + dropout 1.6e-8 / 1.7e-8 /
               1.7e-7 / 3.6e-8 on the four paths; beside a NaN row 1.5e-8 (skinny<8>), 1.8e-7 (MFMA)
  dense_dgrad  skinny<8> 1.1e-7, skinny<16> 3.0e-8, MFMA plain 2.1e-7, MFMA split-K 8.6e-8; gated 8.2e-8 / 1.7e-7 /
               2.5e-8 and with gate_rows = 3 7.0e-8 / 1.2e-7 / 2.5e-8 (skinny / plain / split-K)
  dense_wgrad  skinny dW 1.6e-7, db 6.6e-8; MFMA GN = 7 and 8 dW 8.1e-8, db 3.4e-8; GN = 65 dW 1.8e-7, db 9.6e-8;
               GN = 64 dW 2.1e-7, db 5.1e-8 (all three ways)
  mlp_tail_fwd model chain: layer 0 2.4e-7 (either mode; 1 element of 3584 and 1 of 33280 excluded at M = 7 and 65,
               share 2.8e-4 at most), layers 1-4 1.4e-7 (1 of 16640 excluded in layer 1 at M = 65, share 6.0e-5);
               K0 = 40 chain 1.6e-7 / 1.7e-7; K0 = 520 chain 4.0e-8 / 1.3e-7 (layer 0 / layers 1-4)
  mlp_tail_bwd model widths 2.9e-7, (8, 8, 8, 8, 4) 1.2e-7, (24, 10, 6, 7, 3) 1.2e-7
  rows_wgrad   dW 1.3e-7, db 7.6e-8 over every R and segment
Every bit-identity assertion on mlp_tail_fwd held as stated above.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import rng

gpu = pytest.mark.gpu  # per test: the host-only self-check of the bound lives in this file too

TOL = 1e-5
NAN = float("nan")
SENT = -7.5  # sentinel prefill of guards and of outputs a cleared flag must leave alone
GUARD = 64
SEED, STEP = 11, 5


# ---------------------------------------------------------------------------------------------------- the check
def _within(out, ref, mag):
    """Per-element verdict of the bound (float64 tensors)."""
    return (out - ref).abs() <= TOL * mag


def _check(name, out, ref, mag, excl=None):
    """Finite, within the bound outside `excl` (at most 1 element in 1000); prints and returns the worst err / mag."""
    assert torch.isfinite(out).all(), f"{name}: non-finite output"
    out = out.double()
    ok = _within(out, ref, mag)
    n_ex = 0
    if excl is not None:
        n_ex = int(excl.sum())
        assert n_ex * 1000 <= excl.numel(), f"{name}: {n_ex} of {excl.numel()} elements excluded"
        ok = ok | excl
    live = (mag > 0) if excl is None else ((mag > 0) & ~excl)
    ratio = ((out - ref).abs() / mag.clamp_min(1e-300))[live]
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"[dense_gpu] {name}: worst err/mag {worst:.3e}, excluded {n_ex}/{out.numel()}")
    bad = (~ok).nonzero()
    assert bad.numel() == 0, f"{name}: {bad.shape[0]} elements outside 1e-5 * mag, worst err/mag {worst:.3e}, first at {bad[0].tolist()}"
    return worst


def _mm64(A, B):
    """ref[i][j] = sum_k A[i][k] B[j][k] in float64, and the same on absolute values."""
    A, B = A.double(), B.double()
    return A @ B.T, A.abs() @ B.abs().T


def _finish64(z, mag, relu, keep, scale):
    """(expected, mag, excl) of relu / dropout on the float64 pre-activation z: excl = ReLU decisions within rounding."""
    excl = (z.abs() <= TOL * mag) if relu else None
    e = z.clamp_min(0) if relu else z
    if keep is not None:
        e = torch.where(keep, e * scale, torch.zeros_like(e))
        mag = mag * scale
    return e, mag, excl


def _check_act(name, out, z, mag, relu, keep=None, scale=1.0):
    """An activated layer output: the bound, and with dropout the exact zero pattern."""
    e, m, excl = _finish64(z, mag, relu, keep, scale)
    w = _check(name, out, e, m, excl)
    if keep is not None:
        assert (out[~keep] == 0).all(), f"{name}: a dropped element is not 0.0"
        want = keep & (z > 0) if relu else keep & (z != 0)
        diff = (out != 0) != want
        if excl is not None:
            diff &= ~excl
        assert not diff.any(), f"{name}: zero pattern differs from dropout_keep at {diff.nonzero()[0].tolist()}"
    return w


def _keep(stream, row0, M, N, p):
    return torch.from_numpy(rng.dropout_keep(SEED, stream, STEP, row0, M, N, p))


def _scale(p):
    return float(rng.dropout_scale(p))


def _g(*key):
    return torch.Generator().manual_seed(hash(tuple(int(k) for k in key)) % (1 << 31))


# ---------------------------------------------------------------------------------------------------- cases
FWD_SHAPES = [(1, 4, 1), (8, 2052, 7), (3, 8200, 5),        # skinny<8>: 2nd unrolled step, 2nd outer trip
              (9, 68, 6), (16, 516, 9),                      # skinny<16>
              (7, 30, 5), (16, 67, 33),                      # M <= 16 but K % 4 != 0: MFMA
              (65, 33, 65),                                  # MFMA, one split, ragged in every dimension
              (17, 1000, 66)]                                # MFMA split-K, K no multiple of 32
SPLITK = (17, 1000, 66)
# (scratch floats, max_splits): ample; the 8 splits halve to 2; no split; capped at 2
SPLITK_WAYS = [(1 << 15, 0), (3 * 17 * 66, 0), (0, 0), (1 << 15, 2)]
# relu + dropout on skinny<8>, skinny<16>, plain MFMA, split-K
FWD_DROP = [((8, 2052, 7), 0.3), ((16, 516, 9), 0.5), ((65, 33, 65), 0.3), ((17, 1000, 66), 0.5)]
FWD_ROW0 = 1000

# (M, N, K, scratch floats or None)
DGRAD_CASES = [(2, 4, 5, None), (3, 20, 64, None), (8, 1536, 70, None),      # skinny<8> up to its LDS limit
               (8, 1540, 70, None), (8, 1540, 70, 1 << 15),                  # just past it: MFMA, plain and split-K
               (16, 512, 130, None),                                         # skinny<16> at its limit
               (9, 516, 64, None),                                           # past it: MFMA
               (37, 20, 64, None), (70, 33, 65, None),                       # MFMA plain
               (20, 2048, 64, 1 << 15), (17, 300, 70, 1 << 15),              # split-K (16 and 2 slabs)
               (20, 2048, 64, None)]                                         # the same without scratch: plain
# gate / skip on one case per path: skinny, plain, split-K
DGRAD_PATHS = [(3, 20, 64, None), (37, 20, 64, None), (20, 2048, 64, 1 << 15)]
# gate_rows = 3 with M = 6 on the same three paths (N % 4 != 0 keeps a 6-row case off the skinny kernel)
DGRAD_GATE_ROWS = [(6, 20, 64, None), (6, 30, 64, None), (6, 2050, 64, 1 << 15)]
GSCALE = float(np.float32(1.0 / 0.7))

# (M, N, K, scratch floats, target_blocks)
WGRAD_CASES = [(1, 1, 4, 0, 256), (16, 7, 1028, 0, 256),                     # skinny; K/4 > 256: a 2nd block in x
               (3, 5, 6, 1 << 12, 256), (17, 5, 7, 1 << 12, 256),            # MFMA at tiny M (K % 4 != 0; M > 16)
               (100, 33, 64, 1 << 14, 256),                                  # GN = 65: the bias column opens a tile
               (1000, 20, 63, 1 << 15, 256), (1000, 20, 63, 1 << 15, 1024),  # GN = 64: it closes one; 8 slabs
               (1000, 20, 63, 20 * 64, 256)]                                 # scratch for exactly one slab
WGRAD_SKIP = [(16, 7, 1028, 0, 256), (100, 33, 64, 1 << 14, 256)]

MODEL_CHAIN = (96, (512, 256, 128, 64, 20))
SMALL_CHAIN = (40, (8, 8, 8, 8, 4))
LONG_CHAIN = (520, (8, 8, 8, 8, 4))   # five split-K slabs in mode 1
RAGGED_BWD = (5, (24, 10, 6, 7, 3))   # backward only: inner widths no multiple of 4
CHAIN_M = [1, 7, 9, 65]
CHAIN_RELU = (1, 1, 1, 1, 0)
CHAIN_P = (0.3, 0.2, 0.0, 0.0, 0.0)
CHAIN_STREAM = (rng.S_DET_DROP1, rng.S_DET_DROP2, 0, 0, 0)
CHAIN_ROW0 = 500
CHAIN_GS = tuple(float(np.float32(v)) for v in (1.0 / 0.7, 1.0 / 0.8, 1.0, 1.0))

ROWS_SEGS = [(20, 64, True), (33, 31, True), (1, 32, True), (64, 5, False), (32, 33, True), (7, 1, True)]  # O, I, db
ROWS_R = [1, 3, 17, 70, 640]


@functools.lru_cache(maxsize=None)
def _fwd_case(M, K, N):
    g = _g(1, M, K, N)
    X = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    z, mag = _mm64(X, W)
    return X, W, b, z + b.double(), mag + b.double().abs()


def _gate_like(g, *shape):
    """positive values, negative values and exact zeros"""
    h = torch.randn(*shape, generator=g)
    h[torch.rand(*shape, generator=g) < 0.2] = 0.0
    h.view(-1)[:3] = torch.tensor([0.5, 0.0, -0.5])  # all three kinds even in the smallest gate
    return h


@functools.lru_cache(maxsize=None)
def _dgrad_case(M, N, K, gate_rows=0):
    g = _g(2, M, N, K)
    dY = torch.randn(M, N, generator=g)
    W = torch.randn(N, K, generator=g) / N ** 0.5
    gate = _gate_like(g, gate_rows or M, K)
    ref, mag = _mm64(dY, W.T)
    return dY, W, gate, ref, mag


@functools.lru_cache(maxsize=None)
def _wgrad_case(M, N, K):
    g = _g(3, M, N, K)
    dY = torch.randn(M, N, generator=g)
    X = torch.randn(M, K, generator=g)
    ref, mag = _mm64(dY.T, X.T)
    return dY, X, ref, mag, dY.double().sum(0), dY.double().abs().sum(0)


@functools.lru_cache(maxsize=None)
def _chain_case(K0, widths, M):
    g = _g(4, K0, M, *widths)
    X = torch.randn(M, K0, generator=g)
    Ks = (K0,) + tuple(widths[:-1])
    W = [torch.randn(n, k, generator=g) * (2.0 / k) ** 0.5 for k, n in zip(Ks, widths)]
    b = [0.1 * torch.randn(n, generator=g) for n in widths]
    h = [_gate_like(g, M, n) for n in widths[:4]]
    dout = torch.randn(M, widths[4], generator=g)
    return X, W, b, h, dout


def _chain_layer64(inp, W, b, i, M):
    """float64 layer i of the chain on `inp`: (z, mag, keep, scale)"""
    z, mag = _mm64(inp, W[i])
    z, mag = z + b[i].double(), mag + b[i].double().abs()
    keep = _keep(CHAIN_STREAM[i], CHAIN_ROW0, M, W[i].shape[0], CHAIN_P[i]) if CHAIN_P[i] > 0 else None
    return z, mag, keep, _scale(CHAIN_P[i]) if CHAIN_P[i] > 0 else 1.0


@functools.lru_cache(maxsize=None)
def _rows_case(R, segs):
    g = _g(5, R, len(segs))
    A = [torch.randn(R, O, generator=g) for O, I, _ in segs]
    X = [torch.randn(R, I, generator=g) for O, I, _ in segs]
    return A, X


# ---------------------------------------------------------------------------------------------------- host-only
def _matmul_problems():
    """Every listed shape as (name, A[rows][red], B[cols][red]): all eight kernels compute such a product."""
    for M, K, N in FWD_SHAPES:
        X, W = _fwd_case(M, K, N)[:2]
        yield f"fwd{(M, K, N)}", X, W
    for M, N, K, _ in DGRAD_CASES + DGRAD_GATE_ROWS:
        dY, W = _dgrad_case(M, N, K)[:2]
        yield f"dgrad{(M, N, K)}", dY, W.T.contiguous()
    for M, N, K, _, _ in WGRAD_CASES:
        dY, X = _wgrad_case(M, N, K)[:2]
        yield f"wgrad{(M, N, K)}", dY.T.contiguous(), X.T.contiguous()
    for K0, widths in (MODEL_CHAIN, SMALL_CHAIN, LONG_CHAIN, RAGGED_BWD):
        for M in CHAIN_M:
            X, W, b, h, dout = _chain_case(K0, widths, M)
            yield f"chain{(K0, M)}.fwd0", X, W[0]
            for i in range(1, 5):
                yield f"chain{(K0, M)}.fwd{i}", h[i - 1], W[i]
            yield f"chain{(K0, M)}.bwd4", dout, W[4].T.contiguous()
            for i in range(1, 4):
                yield f"chain{(K0, M)}.bwd{i}", h[i], W[i].T.contiguous()
    for R in ROWS_R:
        A, X = _rows_case(R, tuple(ROWS_SEGS))
        for s, (O, I, _) in enumerate(ROWS_SEGS):
            yield f"rows{(R, O, I)}", A[s].T.contiguous(), X[s].T.contiguous()


def test_bound_has_teeth_on_the_cpu():
    """The bound admits an honest fp32 evaluation of every listed shape and rejects three subtly wrong ones: the last
    element of the reduction dropped, one output column shifted, one split-K slab omitted."""
    n, teeth = 0, [0, 0, 0]
    for name, A, B in _matmul_problems():
        ref, mag = _mm64(A, B)
        assert _within((A @ B.T).double(), ref, mag).all(), f"{name}: fp32 torch outside the bound"
        red = A.shape[1]
        # (the gates hold exact zeros: a left-out term that is zero in every output is no error)
        live = lambda lo, hi: bool((A[:, lo:hi].abs() @ B[:, lo:hi].abs().T).max() > 0)
        if red >= 2 and live(red - 1, red):
            wrong = (A[:, :-1] @ B[:, :-1].T).double()
            assert not _within(wrong, ref, mag).all(), f"{name}: a dropped last element passes"
            teeth[0] += 1
        S = min(8, red)
        lo, hi = (S - 2) * red // S, (S - 1) * red // S  # the slab before the last
        if red >= 2 and live(lo, hi):
            keep = torch.ones(red, dtype=torch.bool)
            keep[lo:hi] = False
            wrong = (A[:, keep] @ B[:, keep].T).double()
            assert not _within(wrong, ref, mag).all(), f"{name}: an omitted split-K slab passes"
            teeth[1] += 1
        if B.shape[0] >= 2:
            wrong = (A @ B.T).double()
            wrong[:, 0] = wrong[:, 1]
            assert not _within(wrong, ref, mag).all(), f"{name}: a shifted column passes"
            teeth[2] += 1
        n += 1
    print(f"[dense_gpu] teeth: {n} shapes, wrong variants rejected {teeth}")
    assert n > 100 and min(teeth) >= 3 * n // 4  # (a 1-long reduction or a single column has no such variant)


def test_relu_exclusions_stay_under_the_cap_on_the_cpu():
    """The float64 reference alone leaves at most 1 ReLU decision in 1000 within rounding of zero, per checked tensor,
    at the seeds used (the chain's layers on the float64 chain's own outputs, which stand in for the device's)."""
    for (M, K, N), p in FWD_DROP:
        z, mag = _fwd_case(M, K, N)[3:]
        assert int((z.abs() <= TOL * mag).sum()) * 1000 <= z.numel(), (M, K, N)
    for K0, widths in (MODEL_CHAIN, SMALL_CHAIN, LONG_CHAIN):
        for M in CHAIN_M:
            X, W, b, _, _ = _chain_case(K0, widths, M)
            inp = X
            for i in range(5):
                z, mag, keep, scale = _chain_layer64(inp, W, b, i, M)
                e, _, excl = _finish64(z, mag, CHAIN_RELU[i], keep, scale)
                if excl is not None:
                    assert int(excl.sum()) * 1000 <= excl.numel(), (K0, M, i)
                inp = e.float()


# ---------------------------------------------------------------------------------------------------- device side
def _nat():
    from vad_amd import _native
    return _native


def _dev():
    return torch.device("cuda")


def _scratch(sf):
    """sf NaN floats and a sentinel guard behind them"""
    s = torch.full((sf + GUARD,), NAN, device=_dev())
    s[sf:] = SENT
    return s


def _guard_ok(s, sf, name):
    assert (s[sf:] == SENT).all(), f"{name}: wrote past its scratch"


def _flag(v):
    return None if v is None else torch.tensor([v], dtype=torch.int32, device=_dev())


def _p(t):
    return None if t is None else t.data_ptr()


def _parr(ts):
    return (ctypes.c_void_p * len(ts))(*[_p(t) for t in ts])


def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


def _dense_fwd(X, W, b, relu=0, p=0.0, stream=0, row0=0, max_splits=0, sf=1 << 15):
    nat, d = _nat(), _dev()
    (M, K), N = X.shape, W.shape[0]
    Xd, Wd, bd = X.to(d), W.to(d), b.to(d)  # the device copies stay alive until the kernel ran
    Y = torch.full((M, N), NAN, device=d)
    scr = _scratch(sf)
    nat.check(nat.lib().vad_dense_forward_ex(_p(Xd), M, K, _p(Wd), _p(bd), N, _p(Y), relu, p, SEED, stream, STEP, row0,
                                             max_splits, _p(scr), sf, nat.stream_of(d)))
    torch.cuda.synchronize()
    _guard_ok(scr, sf, "dense_fwd")
    return Y.cpu()


def _dense_dgrad(dY, W, gate=None, gscale=1.0, gate_rows=0, flag=None, sf=None, fill=NAN):
    nat, d = _nat(), _dev()
    (M, N), K = dY.shape, W.shape[1]
    dYd, Wd, gd, fd = dY.to(d), W.to(d), None if gate is None else gate.to(d), _flag(flag)
    dX = torch.full((M, K), fill, device=d)
    scr = None if sf is None else _scratch(sf)
    nat.check(nat.lib().vad_dense_dgrad(_p(dYd), M, N, _p(Wd), K, _p(dX), _p(gd), gscale, gate_rows, _p(fd), _p(scr),
                                        sf or 0, nat.stream_of(d)))
    torch.cuda.synchronize()
    if scr is not None:
        _guard_ok(scr, sf, "dense_dgrad")
    return dX.cpu()


def _dense_wgrad(dY, X, with_db=True, flag=None, sf=0, target=256, fill=NAN):
    nat, d = _nat(), _dev()
    (M, N), K = dY.shape, X.shape[1]
    dYd, Xd, fd = dY.to(d), X.to(d), _flag(flag)
    dW = torch.full((N * K + GUARD,), fill, device=d)
    db = torch.full((N + GUARD,), fill, device=d)
    dW[N * K:] = SENT
    db[N:] = SENT
    scr = _scratch(sf)
    nat.check(nat.lib().vad_dense_wgrad(_p(dYd), M, N, _p(Xd), K, _p(dW), _p(db) if with_db else None, _p(fd), _p(scr),
                                        sf, target, nat.stream_of(d)))
    torch.cuda.synchronize()
    _guard_ok(scr, sf, "dense_wgrad")
    assert (dW[N * K:] == SENT).all() and (db[N:] == SENT).all(), "dense_wgrad: wrote past dW or db"
    return dW[:N * K].view(N, K).cpu(), db[:N].cpu()


# ---------------------------------------------------------------------------------------------------- dense_fwd
@gpu
@pytest.mark.parametrize("M,K,N", FWD_SHAPES)
def test_dense_fwd_plain_and_relu(M, K, N):
    X, W, b, z, mag = _fwd_case(M, K, N)
    _check(f"dense_fwd{(M, K, N)}", _dense_fwd(X, W, b), z, mag)
    _check_act(f"dense_fwd{(M, K, N)} relu", _dense_fwd(X, W, b, relu=1), z, mag, 1)


@gpu
@pytest.mark.parametrize("sf,max_splits", SPLITK_WAYS)
def test_dense_fwd_splitk_four_ways(sf, max_splits):
    X, W, b, z, mag = _fwd_case(*SPLITK)
    _check(f"dense_fwd{SPLITK} scratch {sf} max_splits {max_splits}", _dense_fwd(X, W, b, max_splits=max_splits, sf=sf),
           z, mag)


@gpu
@pytest.mark.parametrize("shape,p", FWD_DROP)
def test_dense_fwd_relu_dropout(shape, p):
    M, K, N = shape
    X, W, b, z, mag = _fwd_case(M, K, N)
    Y = _dense_fwd(X, W, b, relu=1, p=p, stream=rng.S_DIRECT_DROP1, row0=FWD_ROW0)
    keep = _keep(rng.S_DIRECT_DROP1, FWD_ROW0, M, N, p)
    assert 0 < int(keep.sum()) < keep.numel()
    _check_act(f"dense_fwd{shape} relu dropout {p}", Y, z, mag, 1, keep, _scale(p))


@gpu
@pytest.mark.parametrize("shape", [(8, 2052, 7), (65, 33, 65)])
def test_dense_fwd_nan_row_stays_in_its_row(shape):
    """relu_nan keeps a NaN: the row of Y fed by a NaN in X is NaN, every other row is finite and right"""
    M, K, N = shape
    X, W, b, z, mag = _fwd_case(M, K, N)
    r = M // 2
    Xn = X.clone()
    Xn[r, K - 1] = NAN
    Y = _dense_fwd(Xn, W, b, relu=1)
    assert torch.isnan(Y[r]).all()
    rest = torch.arange(M) != r
    _check_act(f"dense_fwd{shape} NaN row", Y[rest], z[rest], mag[rest], 1)


# ---------------------------------------------------------------------------------------------------- dense_dgrad
def _gated(ref, mag, gate, gscale, gate_rows=0):
    g = gate if not gate_rows else gate[torch.arange(ref.shape[0]) % gate_rows]
    on = g > 0
    return torch.where(on, ref * gscale, torch.zeros_like(ref)), torch.where(on, mag * gscale, torch.zeros_like(mag))


@gpu
@pytest.mark.parametrize("M,N,K,sf", DGRAD_CASES)
def test_dense_dgrad(M, N, K, sf):
    dY, W, _, ref, mag = _dgrad_case(M, N, K)
    _check(f"dense_dgrad{(M, N, K)} scratch {sf}", _dense_dgrad(dY, W, sf=sf), ref, mag)


@gpu
@pytest.mark.parametrize("M,N,K,sf", DGRAD_PATHS)
def test_dense_dgrad_gate(M, N, K, sf):
    dY, W, gate, ref, mag = _dgrad_case(M, N, K)
    assert (gate > 0).any() and (gate < 0).any() and (gate == 0).any()
    e, m = _gated(ref, mag, gate, GSCALE)
    dX = _dense_dgrad(dY, W, gate=gate, gscale=GSCALE, sf=sf)
    _check(f"dense_dgrad{(M, N, K)} gate", dX, e, m)
    assert (dX[~(gate > 0)] == 0).all()


@gpu
@pytest.mark.parametrize("M,N,K,sf", DGRAD_GATE_ROWS)
def test_dense_dgrad_gate_rows(M, N, K, sf):
    """gate_rows = 3 with M = 6: row m is gated by gate row m % 3"""
    dY, W, gate, ref, mag = _dgrad_case(M, N, K, 3)
    assert gate.shape[0] == 3 and not torch.equal(gate[0] > 0, gate[1] > 0)
    e, m = _gated(ref, mag, gate, GSCALE, 3)
    _check(f"dense_dgrad{(M, N, K)} gate_rows 3", _dense_dgrad(dY, W, gate=gate, gscale=GSCALE, gate_rows=3, sf=sf), e, m)


@gpu
@pytest.mark.parametrize("M,N,K,sf", DGRAD_PATHS)
def test_dense_dgrad_skip_flag(M, N, K, sf):
    dY, W, _, ref, mag = _dgrad_case(M, N, K)
    _check(f"dense_dgrad{(M, N, K)} flag 1", _dense_dgrad(dY, W, flag=1, sf=sf), ref, mag)
    assert (_dense_dgrad(dY, W, flag=0, sf=sf, fill=SENT) == SENT).all()


# ---------------------------------------------------------------------------------------------------- dense_wgrad
@gpu
@pytest.mark.parametrize("M,N,K,sf,target", WGRAD_CASES)
@pytest.mark.parametrize("with_db", [True, False])
def test_dense_wgrad(M, N, K, sf, target, with_db):
    """dW and db are written, not accumulated (NaN prefill); a null db leaves the weight gradient alone"""
    dY, X, ref, mag, dbr, dbm = _wgrad_case(M, N, K)
    dW, db = _dense_wgrad(dY, X, with_db=with_db, sf=sf, target=target)
    name = f"dense_wgrad{(M, N, K)} scratch {sf} target {target}"
    _check(name + " dW", dW, ref, mag)
    if with_db:
        _check(name + " db", db, dbr, dbm)
    else:
        assert torch.isnan(db).all()


@gpu
@pytest.mark.parametrize("M,N,K,sf,target", WGRAD_SKIP)
def test_dense_wgrad_skip_flag(M, N, K, sf, target):
    dY, X, ref, mag, dbr, dbm = _wgrad_case(M, N, K)
    dW, db = _dense_wgrad(dY, X, flag=1, sf=sf, target=target)
    _check(f"dense_wgrad{(M, N, K)} flag 1 dW", dW, ref, mag)
    _check(f"dense_wgrad{(M, N, K)} flag 1 db", db, dbr, dbm)
    dW, db = _dense_wgrad(dY, X, flag=0, sf=sf, target=target, fill=SENT)
    assert (dW == SENT).all() and (db == SENT).all()


# ---------------------------------------------------------------------------------------------------- mlp_tail_fwd
def _knobs(rb, wide):
    L = _nat().lib()
    _nat().check(L.vad_set_tuning(b"mlp_tail_rb", rb))
    _nat().check(L.vad_set_tuning(b"mlp_tail_wide", wide))


def _chain_fwd(X, W, b, mode, sf=1 << 19):
    nat, d = _nat(), _dev()
    M, K0 = X.shape
    widths = [w.shape[0] for w in W]
    Xd, Wd, bd = X.to(d), [w.to(d) for w in W], [v.to(d) for v in b]
    out = [torch.full((M, n), NAN, device=d) for n in widths]
    scr = _scratch(sf)
    nat.check(nat.lib().vad_mlp_tail_forward(
        _p(Xd), M, K0, _arr(ctypes.c_int, widths), _parr(Wd), _parr(bd), _arr(ctypes.c_int, CHAIN_RELU),
        _arr(ctypes.c_double, CHAIN_P), _arr(ctypes.c_uint32, CHAIN_STREAM), SEED, STEP, CHAIN_ROW0, mode, _parr(out),
        _p(scr), sf, nat.stream_of(d)))
    torch.cuda.synchronize()
    _guard_ok(scr, sf, "mlp_tail_forward")
    return [o.cpu() for o in out]


@gpu
@pytest.mark.parametrize("M", CHAIN_M)
@pytest.mark.parametrize("chain", [MODEL_CHAIN, SMALL_CHAIN, LONG_CHAIN], ids=["model", "small", "long"])
def test_mlp_tail_forward(chain, M):
    K0, widths = chain
    X, W, b, _, _ = _chain_case(K0, widths, M)
    auto = 4 if M >= 64 else 8
    try:
        for mode in (0, 1):
            got = {}
            for wide in (0, 1):
                for rb in (0, 2, 4, 8):
                    _knobs(rb, wide)
                    got[wide, rb] = outs = _chain_fwd(X, W, b, mode)
                    inp = X
                    for i in range(5):
                        z, mag, keep, scale = _chain_layer64(inp, W, b, i, M)
                        _check_act(f"mlp_tail_fwd K0 {K0} M {M} mode {mode} wide {wide} rb {rb} layer {i}", outs[i],
                                   z, mag, CHAIN_RELU[i], keep, scale)
                        inp = outs[i]  # the next layer is judged on what the device fed it
            # rows are independent and the K-slices depend on the thread count only (module docstring)
            same = lambda a, c: all(torch.equal(u, v) for u, v in zip(got[a], got[c]))
            assert same((0, 2), (0, 4)) and same((0, 2), (0, 8)), "256 threads: rb 2 / 4 / 8 differ"
            assert same((1, 2), (1, 4)), "1024 threads: rb 2 / 4 differ"
            assert same((1, 8), (0, 8)), "rb 8 runs one kernel under either mlp_tail_wide"
            assert same((0, 0), (0, auto)) and same((1, 0), (1, auto)), "rb 0 is not the rb it picks"
    finally:
        _knobs(0, 1)


# ---------------------------------------------------------------------------------------------------- mlp_tail_bwd
def _chain_bwd(K0, widths, M, W, h, dout, flag=None, fill=NAN):
    nat, d = _nat(), _dev()
    Ks = [K0] + list(widths[:-1])
    Wd, hd, dd, fd = [w.to(d) for w in W], [v.to(d) for v in h], dout.to(d), _flag(flag)
    dbuf = [torch.full((M * n + GUARD,), fill, device=d) for n in widths[:4]]
    for t, n in zip(dbuf, widths[:4]):
        t[M * n:] = SENT
    nat.check(nat.lib().vad_mlp_tail_backward(M, _p(dd), _parr(Wd), _arr(ctypes.c_int, Ks), _arr(ctypes.c_int, widths),
                                              _parr(hd), _arr(ctypes.c_float, CHAIN_GS), _parr(dbuf), _p(fd),
                                              nat.stream_of(d)))
    torch.cuda.synchronize()
    for t, n in zip(dbuf, widths[:4]):
        assert (t[M * n:] == SENT).all(), "mlp_tail_backward: wrote past a gradient"
    return [t[:M * n].view(M, n).cpu() for t, n in zip(dbuf, widths[:4])]


@gpu
@pytest.mark.parametrize("M", CHAIN_M)
@pytest.mark.parametrize("chain", [MODEL_CHAIN, SMALL_CHAIN, RAGGED_BWD], ids=["model", "small", "ragged"])
def test_mlp_tail_backward(chain, M):
    """d[i-1] = (d[i] W[i]) * (h[i-1] > 0 ? gscale[i-1] : 0), each layer against float64 of the device's own d[i].
    The ragged chain (24, 10, 6, 7, 3) reads pad columns the kernel now zeroes; a pass here cannot prove the code before
    that wrong (module docstring)."""
    K0, widths = chain
    _, W, _, h, dout = _chain_case(K0, widths, M)
    assert all((v > 0).any() and (v == 0).any() for v in h) and any((v < 0).any() for v in h)
    for flag in (None, 1):
        dg = _chain_bwd(K0, widths, M, W, h, dout, flag=flag)
        up = dout
        for i in range(4, 0, -1):
            ref, mag = _mm64(up, W[i].T)
            e, m = _gated(ref, mag, h[i - 1], CHAIN_GS[i - 1])
            _check(f"mlp_tail_bwd widths {widths} M {M} flag {flag} d[{i - 1}]", dg[i - 1], e, m)
            assert (dg[i - 1][~(h[i - 1] > 0)] == 0).all()
            up = dg[i - 1]
    assert all((t == SENT).all() for t in _chain_bwd(K0, widths, M, W, h, dout, flag=0, fill=SENT))


# ---------------------------------------------------------------------------------------------------- rows_wgrad
def _rows_wgrad(R, segs, A, X, flag=None, fill=NAN):
    nat, d = _nat(), _dev()
    Ad, Xd, fd = [t.to(d) for t in A], [t.to(d) for t in X], _flag(flag)
    dW = [torch.full((O * I + GUARD,), fill, device=d) for O, I, _ in segs]
    db = [torch.full((O + GUARD,), fill, device=d) for O, I, _ in segs]
    for (O, I, _), w, v in zip(segs, dW, db):
        w[O * I:] = SENT
        v[O:] = SENT
    nat.check(nat.lib().vad_rows_wgrad(R, len(segs), _parr(dW), _parr([v if s[2] else None for s, v in zip(segs, db)]),
                                       _parr(Ad), _parr(Xd), _arr(ctypes.c_int, [s[0] for s in segs]),
                                       _arr(ctypes.c_int, [s[1] for s in segs]), _p(fd), nat.stream_of(d)))
    torch.cuda.synchronize()
    for (O, I, _), w, v in zip(segs, dW, db):
        assert (w[O * I:] == SENT).all() and (v[O:] == SENT).all(), f"rows_wgrad: wrote past dW or db of {(O, I)}"
    return [w[:O * I].view(O, I).cpu() for (O, I, _), w in zip(segs, dW)], [v[:O].cpu() for (O, I, _), v in zip(segs, db)]


def _rows_check(R, segs, A, X, dW, db, tag):
    for s, (O, I, has_db) in enumerate(segs):
        ref, mag = _mm64(A[s].T, X[s].T)
        _check(f"rows_wgrad R {R} seg {(O, I)} {tag} dW", dW[s], ref, mag)
        if has_db:
            _check(f"rows_wgrad R {R} seg {(O, I)} {tag} db", db[s], A[s].double().sum(0), A[s].double().abs().sum(0))
        else:
            assert torch.isnan(db[s]).all()


@gpu
@pytest.mark.parametrize("R", ROWS_R)
def test_rows_wgrad_six_segments(R):
    """The bias is column I of a segment's tiles: the last column of a tile at I = 31, the first of a new one at 32"""
    segs = tuple(ROWS_SEGS)
    A, X = _rows_case(R, segs)
    for flag in (None, 1):
        dW, db = _rows_wgrad(R, segs, A, X, flag=flag)
        _rows_check(R, segs, A, X, dW, db, f"flag {flag}")
    dW, db = _rows_wgrad(R, segs, A, X, flag=0, fill=SENT)
    assert all((t == SENT).all() for t in dW + db)


@gpu
def test_rows_wgrad_single_segment():
    segs = ((33, 31, True),)
    A, X = _rows_case(17, segs)
    dW, db = _rows_wgrad(17, segs, A, X)
    _rows_check(17, segs, A, X, dW, db, "alone")
