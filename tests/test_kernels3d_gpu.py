"""Single-kernel parity of the 3-D clip building blocks (conv3d.hip, conv3d_direct.hip, the conv3s2_* implicit GEMMs,
conv3d_x3_fwd) at ragged shapes: odd extents, partial tiles, empty parity classes, pooling windows and bins that do not
divide the volume.  Every reference is float64 torch on the CPU.

Conv bound: |out - ref64| <= 1e-5 * mag per element, mag = the same operation on the absolute values of the operands
(the "fp32 accumulation level" of test_conv3x3_bf16_mode_matches_rounded_fp64).  A dropped tap or a border off by one
is an error of 1/K of mag or more (K = 27 Ci <= 864 taps here, i.e. >= 1e-3).  Outputs are prefilled with NaN, so an
element no thread wrote fails the finiteness check.  Each case runs on the im2col path (0) and on its fast path; both
must meet the bound, not merely agree."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
CONV_TOL = 1e-5
NCDHW, NDHWC = 0, 1


def _nat():
    from vad_amd import _native
    return _native


def _dev(t):
    return t.contiguous().to("cuda")


def _to_ndhwc(t):   # (N, C, D, H, W) -> (N, D, H, W, C)
    return t.permute(0, 2, 3, 4, 1).contiguous()


def _from_ndhwc(t):
    return t.permute(0, 4, 1, 2, 3).contiguous()


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _ratio(out, ref, mag, label):
    """worst |out - ref| / mag over the elements (mag == 0: the element must be exact)"""
    out = out.double()
    assert out.shape == ref.shape, (label, out.shape, ref.shape)
    assert bool(torch.isfinite(out).all()), f"{label}: non-finite (unwritten?) output elements"
    err = (out - ref).abs()
    zero = mag == 0
    assert bool((err[zero] == 0).all()), f"{label}: non-zero where the operands are all zero"
    r = float((err[~zero] / mag[~zero]).max()) if bool((~zero).any()) else 0.0
    print(f"{label}: worst |err|/mag = {r:.3e}")
    return r


# ------------------------------------------------------------------------------------------------------- convolutions
# (N, Ci, Co, D, H, W, stride (d, h, w), source layout, fast path)
S1, S2 = (1, 1, 1), (2, 2, 2)
CONV_CASES = [
    # direct path (1), stride 1
    (2, 1, 8, 3, 9, 17, S1, NCDHW, 1),     # one past the 2 x 8 x 16 tile on every axis
    (1, 8, 16, 5, 7, 19, S1, NDHWC, 1),
    (2, 16, 32, 1, 8, 16, S1, NDHWC, 1),   # D = 1, an exact H x W tile
    (1, 3, 8, 2, 5, 3, S1, NCDHW, 1),      # below a tile
    # stride-2 implicit GEMMs (2)
    (2, 16, 32, 5, 9, 7, S2, NDHWC, 2),    # all odd
    (2, 16, 32, 4, 8, 6, S2, NDHWC, 2),    # all even: the odd classes' half + 1 tap reads dY index OD -> zero
    (1, 32, 64, 1, 3, 3, S2, NDHWC, 2),    # empty parity classes (pd = 1)
    (3, 16, 32, 2, 1, 5, S2, NDHWC, 2),    # empty parity classes (ph = 1)
    (2, 32, 64, 3, 12, 10, S2, NDHWC, 2),  # mixed
    # the a2 stem geometry: stride (1, 2, 2), 3 channels, from the NCDHW clip (im2col only)
    (2, 3, 16, 5, 37, 27, (1, 2, 2), NCDHW, 0),
    # depth-tap split-bf16 conv (3), forward only
    (2, 32, 64, 3, 18, 22, S1, NDHWC, 3),
    (1, 32, 64, 1, 4, 4, S1, NDHWC, 3),
    (3, 32, 64, 2, 9, 33, S1, NDHWC, 3),
    (2, 32, 64, 5, 20, 13, S1, NDHWC, 3),  # the <2, 8, 16> tile (W <= 16, H > 8): 10 frames in pairs, ragged rows
]
CONV_RUNS = [(c, p) for c in CONV_CASES for p in sorted({0, c[8]})]
CONV_IDS = ["n{}_ci{}_co{}_{}x{}x{}_s{}{}{}_path{}".format(*c[:6], *c[6], p) for c, p in CONV_RUNS]


@functools.lru_cache(maxsize=None)
def _conv_ref(case):
    """float64 operands and references of one case (computed once, shared by both paths, never modified)"""
    N, Ci, Co, D, H, W, s, _, _ = case
    g = torch.Generator().manual_seed(int(np.dot(case[:6], [1, 7, 31, 101, 211, 401])))
    x = torch.randn(N, Ci, D, H, W, generator=g)
    w = torch.randn(Co, Ci, 3, 3, 3, generator=g) / (27 * Ci) ** 0.5
    b = torch.randn(Co, generator=g)
    x64, w64, b64 = x.double(), w.double(), b.double()
    y = F.conv3d(x64, w64, b64, stride=s, padding=1)
    dy = torch.randn(y.shape, generator=g)
    gate = torch.randn(x.shape, generator=g)
    gate[torch.rand(x.shape, generator=g) < 0.25] = 0.0   # exact zeros beside the negative values
    dy64 = dy.double()
    r = dict(x=x, w=w, b=b, dy=dy, gate=gate, y=y, ymag=F.conv3d(x64.abs(), w64.abs(), b64.abs(), stride=s, padding=1),
             dx=torch.nn.grad.conv3d_input(x.shape, w64, dy64, stride=s, padding=1),
             dxmag=torch.nn.grad.conv3d_input(x.shape, w64.abs(), dy64.abs(), stride=s, padding=1),
             dw=torch.nn.grad.conv3d_weight(x64, w.shape, dy64, stride=s, padding=1),
             dwmag=torch.nn.grad.conv3d_weight(x64.abs(), w.shape, dy64.abs(), stride=s, padding=1),
             db=dy64.sum((0, 2, 3, 4)), dbmag=dy64.abs().sum((0, 2, 3, 4)))
    return r


def _scratch(nat, kind, path, case):
    N, Ci, Co, D, H, W, s, _, _ = case
    need = nat.lib().vad_conv3d_scratch_floats(kind, path, N, Ci, D, H, W, Co, *s)
    assert need >= 0, nat.lib().vad_last_error()
    # room for the split-K slabs the plans give the same kernels; NaN so a slab read before it is written shows
    return _nan(need + (1 << 20))


@pytest.mark.parametrize("case,path", CONV_RUNS, ids=CONV_IDS)
def test_conv3d_forward(case, path):
    nat = _nat()
    N, Ci, Co, D, H, W, s, layout, _ = case
    r = _conv_ref(case)
    x = _dev(r["x"] if layout == NCDHW else _to_ndhwc(r["x"]))
    w, b = _dev(r["w"]), _dev(r["b"])
    OD, OH, OW = r["y"].shape[2:]
    y = _nan(N, OD, OH, OW, Co)
    sc = _scratch(nat, 0, path, case)
    nat.check(nat.lib().vad_conv3d_forward(x.data_ptr(), layout, N, Ci, D, H, W, w.data_ptr(), b.data_ptr(), Co, *s,
                                           path, y.data_ptr(), sc.data_ptr(), sc.numel(), nat.stream_of(x.device)))
    torch.cuda.synchronize()
    assert _ratio(_from_ndhwc(y.cpu()), r["y"], r["ymag"], f"conv3d fwd path {path}") <= CONV_TOL


@pytest.mark.parametrize("case,path", [(c, p) for c, p in CONV_RUNS if p != 3],
                         ids=[i for i, (c, p) in zip(CONV_IDS, CONV_RUNS) if p != 3])
def test_conv3d_dgrad(case, path):
    """Input gradient; on the stride-2 path also with the fused ReLU gate (exact zeros where !(gate > 0)).  The direct
    path's input gradient is its forward kernel over dY, which writes 8, 16 or 32 channels: other Ci are refused."""
    nat = _nat()
    N, Ci, Co, D, H, W, s, _, _ = case
    r = _conv_ref(case)
    dy, w = _dev(_to_ndhwc(r["dy"])), _dev(r["w"])
    sc = _scratch(nat, 0 if path == 1 else 1, path, case)   # (the direct path sizes both kinds alike; kind 1 refuses Ci)
    for gated in ([0, 1] if path == 2 else [0]):
        dx = _nan(N, D, H, W, Ci)
        gate = _dev(_to_ndhwc(r["gate"])) if gated else None
        rc = nat.lib().vad_conv3d_dgrad(dy.data_ptr(), N, Ci, D, H, W, w.data_ptr(), Co, *s, path, nat.ptr(gate),
                                        dx.data_ptr(), sc.data_ptr(), sc.numel(), nat.stream_of(dy.device))
        if path == 1 and Ci not in (8, 16):
            assert rc != 0 and b"input gradient needs Ci in {8, 16}" in nat.lib().vad_last_error()
            return
        nat.check(rc)
        torch.cuda.synchronize()
        keep = (r["gate"] > 0).double() if gated else 1.0
        assert _ratio(_from_ndhwc(dx.cpu()), r["dx"] * keep, r["dxmag"] * keep,
                      f"conv3d dgrad path {path} gate {gated}") <= CONV_TOL


@pytest.mark.parametrize("case,path", [(c, p) for c, p in CONV_RUNS if p != 3],
                         ids=[i for i, (c, p) in zip(CONV_IDS, CONV_RUNS) if p != 3])
def test_conv3d_wgrad(case, path):
    """Weight and bias gradient (the stride-2 path's db is one more GEMM column; also run without it)."""
    nat = _nat()
    N, Ci, Co, D, H, W, s, layout, _ = case
    r = _conv_ref(case)
    x = _dev(r["x"] if layout == NCDHW else _to_ndhwc(r["x"]))
    dy = _dev(_to_ndhwc(r["dy"]))
    sc = _scratch(nat, 2, path, case)
    for with_db in ([1, 0] if path == 2 else [1]):
        dW, db = _nan(Co, Ci, 3, 3, 3), _nan(Co)
        nat.check(nat.lib().vad_conv3d_wgrad(x.data_ptr(), layout, dy.data_ptr(), N, Ci, D, H, W, Co, *s, path,
                                             dW.data_ptr(), db.data_ptr() if with_db else None, sc.data_ptr(),
                                             sc.numel(), nat.stream_of(x.device)))
        torch.cuda.synchronize()
        assert _ratio(dW.cpu(), r["dw"], r["dwmag"], f"conv3d wgrad path {path} db {with_db}") <= CONV_TOL
        if with_db:
            assert _ratio(db.cpu(), r["db"], r["dbmag"], f"conv3d bias grad path {path}") <= CONV_TOL


# ----------------------------------------------------------------------------------------------------------- MaxPool3d
POOL_CASES = [(2, 8, 5, 9, 7), (2, 16, 5, 9, 7), (3, 8, 4, 8, 8), (1, 32, 1, 3, 2)]
POOL_WINDOWS = [(1, 2, 2), (2, 2, 2)]


def _pool_fwd(nat, y, stats, relu, shape, k):
    N, C, D, H, W = shape
    out = _nan(N, D // k[0], H // k[1], W // k[2], C)
    nat.check(nat.lib().vad_maxpool3d_forward(y.data_ptr(), nat.ptr(stats), relu, N, C, D, H, W, *k, out.data_ptr(),
                                              nat.stream_of(y.device)))
    torch.cuda.synchronize()
    return _from_ndhwc(out.cpu())


def _pool_bwd(nat, y, stats, relu, shape, k, dout, win):
    N, C, D, H, W = shape
    dA = _nan(N, D, H, W, C)
    nat.check(nat.lib().vad_set_tuning(b"maxpool3d_bwd_win", win))
    try:
        nat.check(nat.lib().vad_maxpool3d_backward(y.data_ptr(), nat.ptr(stats), relu, N, C, D, H, W, *k,
                                                   dout.data_ptr(), dA.data_ptr(), nat.stream_of(y.device)))
        torch.cuda.synchronize()
    finally:
        nat.check(nat.lib().vad_set_tuning(b"maxpool3d_bwd_win", 1))
    return _from_ndhwc(dA.cpu())


def _pool_autograd(a, k, dout):
    """torch CPU max_pool3d forward and its gradient w.r.t. the pool's input a (the kernel's dA: the activation's own
    backward is the caller's)"""
    a = a.detach().clone().requires_grad_(True)
    out = F.max_pool3d(a, k)
    out.backward(dout)
    return out.detach(), a.grad


def _pool_relu_check(shape, k, y):
    nat = _nat()
    N, C, D, H, W = shape
    g = torch.Generator().manual_seed(7)
    yd = _dev(_to_ndhwc(y))
    if min(D // k[0], H // k[1], W // k[2]) == 0:   # the window fits nowhere: nothing to write, a zero gradient
        assert _pool_fwd(nat, yd, None, 1, shape, k).numel() == 0
        dout = torch.empty(0, device="cuda")
        for win in (1, 0):
            assert bool((_pool_bwd(nat, yd, None, 1, shape, k, dout, win) == 0).all())
        return None
    dout = torch.randn(N, C, D // k[0], H // k[1], W // k[2], generator=g)
    ref, gref = _pool_autograd(F.relu(y), k, dout)
    out = _pool_fwd(nat, yd, None, 1, shape, k)
    assert torch.equal(out.isnan(), ref.isnan()) and torch.equal(out.nan_to_num(7.0), ref.nan_to_num(7.0))
    dd = _dev(_to_ndhwc(dout))
    for win in (1, 0):
        dA = _pool_bwd(nat, yd, None, 1, shape, k, dd, win)
        assert bool(torch.isfinite(dA).all()), "unwritten dA elements"
        assert torch.equal(dA, gref), f"maxpool3d_bwd_win={win}: {int((dA != gref).sum())} elements differ"
    return ref


@pytest.mark.parametrize("k", POOL_WINDOWS, ids=["k122", "k222"])
@pytest.mark.parametrize("shape", POOL_CASES, ids=["x".join(map(str, s)) for s in POOL_CASES])
def test_maxpool3d_relu_is_bit_equal_to_torch(shape, k):
    """relu = 1, no stats: forward == F.max_pool3d(F.relu(y)) and the backward == torch CPU autograd at the pool's
    input, bit for bit, for both backward kernels.  Standard-normal inputs leave whole windows tied at zero after the
    ReLU, so torch's first-maximum rule decides where the gradient goes; elements outside every complete window (odd
    extents) must be zero."""
    # (seed offset 1: checked on the CPU to leave at least one all-negative window in every case, the 32-window one too)
    y = torch.randn(shape, generator=torch.Generator().manual_seed(1 + sum(shape) + k[0]))
    ref = _pool_relu_check(shape, k, y)
    if ref is not None:
        assert bool((ref == 0).any()), "no all-tied window in this case: the first-maximum rule is not exercised"


@pytest.mark.parametrize("k", POOL_WINDOWS, ids=["k122", "k222"])
def test_maxpool3d_nan_window(k):
    """A window holding a NaN pools to NaN, and its gradient goes to the NaN (the last one in scan order: torch's
    `val > max || isnan(val)`)."""
    shape = POOL_CASES[0]
    y = torch.randn(shape, generator=torch.Generator().manual_seed(3))
    y[0, 1, 0, 2, 3] = float("nan")                 # one NaN in its window
    y[1, 5, 2, 4, 0] = y[1, 5, 2, 5, 1] = float("nan")   # two in one window: the later one takes the gradient
    ref = _pool_relu_check(shape, k, y)
    assert bool(ref[0, 1, 0, 1, 1].isnan()) and bool(ref[1, 5, 2 // k[0], 2, 0].isnan()) and int(ref.isnan().sum()) == 2
    nat = _nat()
    dout = torch.ones(shape[0], shape[1], shape[2] // k[0], shape[3] // k[1], shape[4] // k[2])
    for win in (1, 0):
        dA = _pool_bwd(nat, _dev(_to_ndhwc(y)), None, 1, shape, k, _dev(_to_ndhwc(dout)), win)
        assert float(dA[0, 1, 0, 2, 3]) == 1.0 and float(dA[1, 5, 2, 5, 1]) == 1.0 and float(dA[1, 5, 2, 4, 0]) == 0.0


def _pool_stats_case(shape, k):
    """relu(scale * y + shift) pooling: operands, the float64 reference, the error bound per window and the windows
    whose maximum is decided by more than that bound"""
    N, C, D, H, W = shape
    g = torch.Generator().manual_seed(11 + sum(shape) + k[0])
    y = torch.randn(shape, generator=g)
    stats = torch.randn(4 * C, generator=g)
    sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    stats[2 * C:3 * C] = sign * (0.5 + torch.rand(C, generator=g))    # scale: both signs
    stats[3 * C:] = 0.5 + torch.rand(C, generator=g)                  # shift: most activations above the ReLU's zero
    sc = stats[2 * C:3 * C].double().view(1, C, 1, 1, 1)
    sh = stats[3 * C:].double().view(1, C, 1, 1, 1)
    a = F.relu(sc * y.double() + sh)
    OD, OH, OW = D // k[0], H // k[1], W // k[2]
    dout = torch.randn(N, C, OD, OH, OW, generator=g)
    ref, gref = _pool_autograd(a, k, dout.double())
    # one fused multiply-add and a max: each activation is within 2^-24 of |scale y| + |shift|; 1e-6 of the largest
    # such magnitude in the window bounds the pooled value whichever element wins on the device
    bound = 1e-6 * F.max_pool3d((sc * y.double()).abs() + sh.abs(), k)
    wins = a[:, :, :OD * k[0], :OH * k[1], :OW * k[2]].reshape(N, C, OD, k[0], OH, k[1], OW, k[2])
    top = wins.permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(N, C, OD, OH, OW, -1).topk(2, dim=-1).values
    decided = (top[..., 0] - top[..., 1]) > bound
    return y, stats, dout, ref, gref, bound, decided


STATS_RUNS = [(s, k) for s in POOL_CASES for k in POOL_WINDOWS if min(s[2] // k[0], s[3] // k[1], s[4] // k[2]) > 0]


@pytest.mark.parametrize("shape,k", STATS_RUNS,
                         ids=["{}_k{}".format("x".join(map(str, s)), "".join(map(str, k))) for s, k in STATS_RUNS])
def test_maxpool3d_with_stats_matches_float64(shape, k):
    """The BatchNorm affine + ReLU fused into the pool: forward within 1e-6 (|scale y| + |shift|) of float64; the
    backward equal to float64 autograd wherever the float64 maximum beats the runner-up by more than that margin (at
    most 1 % of the windows are left out), and zero outside the complete windows."""
    nat = _nat()
    y, stats, dout, ref, gref, bound, decided = _pool_stats_case(shape, k)
    left_out = 1.0 - float(decided.double().mean())
    print(f"maxpool stats {shape} {k}: {left_out:.4%} of the windows undecided")
    assert left_out <= 0.01
    yd, sd = _dev(_to_ndhwc(y)), _dev(stats)
    out = _pool_fwd(nat, yd, sd, 1, shape, k).double()
    assert bool(torch.isfinite(out).all())
    print(f"maxpool stats fwd: worst |err|/bound = {float(((out - ref).abs() / bound).max()):.3e}")
    assert bool(((out - ref).abs() <= bound).all())
    mask = torch.ones(shape, dtype=torch.bool)   # elements of decided windows, and everything outside the windows
    m = decided
    for ax, kk in zip((2, 3, 4), k):
        m = m.repeat_interleave(kk, dim=ax)
    mask[:, :, :m.shape[2], :m.shape[3], :m.shape[4]] = m
    for win in (1, 0):
        dA = _pool_bwd(nat, yd, sd, 1, shape, k, _dev(_to_ndhwc(dout)), win).double()
        assert bool(torch.isfinite(dA).all()), "unwritten dA elements"
        assert torch.equal(dA[mask], gref[mask]), f"maxpool3d_bwd_win={win}"


# --------------------------------------------------------------------------------------------------- AdaptiveAvgPool3d
AVG_RUNS = [(s, b) for s in [(2, 64, 1, 1, 1), (2, 64, 3, 5, 7), (1, 32, 2, 6, 5)]
            for b in [(1, 1, 1), (1, 4, 4), (4, 4, 4)]]
AVG_RUNS += [((2, 32, 13, 11, 9), (1, 1, 1)), ((2, 32, 13, 11, 9), (1, 4, 4)),   # block-per-bin kernel (>= 64 voxels/bin)
             ((1, 96, 5, 5, 3), (1, 1, 1))]                                      # ... and its second 64-channel chunk


@pytest.mark.parametrize("shape,bins", AVG_RUNS,
                         ids=["{}_b{}".format("x".join(map(str, s)), "".join(map(str, b))) for s, b in AVG_RUNS])
def test_adaptive_avgpool3d(shape, bins):
    """Forward within 1e-5 of the bin's mean |x|; backward (plain, and gated by a tensor with exact zeros and negative
    values) within 1e-5 of the same operation on |dout|, against float64 autograd."""
    nat = _nat()
    N, C, D, H, W = shape
    g = torch.Generator().manual_seed(sum(shape) * 8 + sum(bins))
    x = torch.randn(shape, generator=g)
    dout = torch.randn(N, C, *bins, generator=g)
    gate = torch.randn(shape, generator=g)
    gate[torch.rand(shape, generator=g) < 0.25] = 0.0
    x64 = x.double().requires_grad_(True)
    ref = F.adaptive_avg_pool3d(x64, bins)
    ref.backward(dout.double())
    xa = x.double().abs().requires_grad_(True)
    mag = F.adaptive_avg_pool3d(xa, bins)
    mag.backward(dout.double().abs())
    xd = _dev(_to_ndhwc(x))
    out = _nan(N, C, *bins)
    st = nat.stream_of(xd.device)
    nat.check(nat.lib().vad_adaptive_avgpool3d_forward(xd.data_ptr(), None, 0, N, C, D, H, W, *bins, out.data_ptr(), st))
    torch.cuda.synchronize()
    assert _ratio(out.cpu(), ref.detach(), mag.detach(), "adaptive avgpool fwd") <= 1e-5
    # relu = 1 (ReLU on load, no BatchNorm statistics: the bbox scorer's call) on the same input -- about half of it is
    # negative -- and with one NaN voxel, which has to reach exactly the bins that hold it
    out = _nan(N, C, *bins)
    nat.check(nat.lib().vad_adaptive_avgpool3d_forward(xd.data_ptr(), None, 1, N, C, D, H, W, *bins, out.data_ptr(), st))
    torch.cuda.synchronize()
    assert float((x < 0).float().mean()) > 0.3
    rref = F.adaptive_avg_pool3d(F.relu(x.double()), bins)
    assert _ratio(out.cpu(), rref, rref, "adaptive avgpool fwd relu") <= 1e-5
    xn = x.clone()
    xn[N - 1, C // 2, D // 2, H // 2, W // 2] = float("nan")
    want = torch.isnan(F.adaptive_avg_pool3d(F.relu(xn.double()), bins))
    assert 1 <= int(want.sum()) < want.numel()
    out = _nan(N, C, *bins)
    nat.check(nat.lib().vad_adaptive_avgpool3d_forward(_dev(_to_ndhwc(xn)).data_ptr(), None, 1, N, C, D, H, W, *bins,
                                                       out.data_ptr(), st))
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.equal(torch.isnan(got), want), "relu = 1: the NaN voxel's bins"
    assert bool(((got.double() - rref).abs()[~want] <= 1e-5 * rref[~want]).all()), "relu = 1: the bins without the NaN"
    dd = _dev(dout)
    for gated in (0, 1):
        gd = _dev(_to_ndhwc(gate)) if gated else None
        dx = _nan(N, D, H, W, C)
        nat.check(nat.lib().vad_adaptive_avgpool3d_backward(dd.data_ptr(), N, C, D, H, W, *bins, nat.ptr(gd),
                                                            dx.data_ptr(), st))
        torch.cuda.synchronize()
        keep = (gate > 0).double() if gated else 1.0
        assert _ratio(_from_ndhwc(dx.cpu()), x64.grad * keep, xa.grad * keep,
                      f"adaptive avgpool bwd gate {gated}") <= 1e-5
