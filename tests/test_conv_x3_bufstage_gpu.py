"""Buffer-resource staging of the split-bf16 3x3 conv kernels (conv3x3_x3_kernel, conv3x3_x3p_kernel in conv_x3.hip):
bit-identity to the kernels before that change, and the zero padding under BN on load.

The move to buffer loads / stores changed how a piece is addressed and masked, never a value that enters an MFMA, so
every output -- raw conv outputs, the forward's BN partial sums, the input gradient's fused BN-backward partials -- must
equal, bit for bit, what commit dfe6ff0 (the parent of the change) computes at the same inputs.  tests/golden/
conv_x3_bufstage.npz holds that record, made with dfe6ff0's kernels (its libvadhip.so plus the two entry points this
test calls, vad_conv3x3_forward_bn and vad_conv3x3_dgrad_bnfuse, which only pass arguments to conv3_fwd / conv3_dgrad)
by record().  The full arrays would take 3 MB, so the record keeps, per array, the SHA-256 of its bytes -- equal digests
are equal bits -- and, to say where a difference lies, the wrapping sum of the 32-bit patterns of every (image, row).

Inputs are small integers over a power of two, drawn from numpy's PCG64 `integers`, so they do not depend on a library's
normal sampler.

Shapes (NF x H x W, Ci -> Co): the smallest that reach each mask of each kernel arm.  3x9x11 at 32 -> 32 has more patch
blocks than BN partial rows, which keeps its forward on the GEMM path (its input gradient is the split kernel); 3x9x13 is
added beside it as the forward that does reach the pipelined kernel's 2 x 8x16 tiles with a half-empty image pair.
"""
import hashlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GOLDEN = __file__.rsplit("/", 1)[0] + "/golden/conv_x3_bufstage.npz"

# (name, NF, Ci, Co, IH, IW, stride)
CASES = [("s1_32_3x9x11", 3, 32, 32, 9, 11, 1),      # partial tile both ways, NF not a multiple of NI (input gradient)
         ("s1_32_3x9x13", 3, 32, 32, 9, 13, 1),      # the same on the pipelined forward (x3p, WCH = 2)
         ("s1_32_1x8x32", 1, 32, 32, 8, 32, 1),      # exact tile: only the halo is masked
         ("s1_64_5x15x15", 5, 64, 64, 15, 15, 1),    # 16x16 tile with one padded row and column
         ("s1_64_2x29x29", 2, 64, 64, 29, 29, 1),
         ("s1_256_5x8x8", 5, 256, 256, 8, 8, 1),     # image mask img0 + im < NF with a partial image group
         ("s2_32_3x57x57", 3, 32, 64, 57, 57, 2),    # odd input size, last output row and column
         ("s2_32_2x10x7", 2, 32, 64, 10, 7, 2)]      # narrower than a tile, row wrap left and right
CASE3D = ("kd3_32_1x3x9x9", 1, 32, 64, 3, 9, 9)     # depth slices 0 and D - 1 mask the kd taps


def _lib():
    from vad_amd import _native
    return _native


def _ints(rng, shape, scale):
    return torch.from_numpy((rng.integers(-(1 << 12), 1 << 12, size=shape).astype(np.float32) * np.float32(scale)))


def _inputs(case):
    name, NF, Ci, Co, IH, IW, s = case
    rng = np.random.Generator(np.random.PCG64(sum(map(ord, name))))
    OH, OW = (IH - 1) // s + 1, (IW - 1) // s + 1
    x = _ints(rng, (NF, IH, IW, Ci), 2.0 ** -11)
    w = _ints(rng, (Co, Ci, 3, 3), 2.0 ** -12 / (9 * Ci) ** 0.5)
    bias = _ints(rng, (Co,), 2.0 ** -12)
    # BN state of the layer that made x: [mean | invstd | scale | shift]; every shift > 0, so a padded tap that lost
    # its mask would enter as relu(shift) > 0
    stats = torch.cat([_ints(rng, (Ci,), 2.0 ** -13), _ints(rng, (Ci,), 2.0 ** -12).abs() + 0.5,
                       _ints(rng, (Ci,), 2.0 ** -11), _ints(rng, (Ci,), 2.0 ** -13).abs() + 0.125])
    dy = _ints(rng, (NF, OH, OW, Co), 2.0 ** -11)
    return dict(x=x, w=w, bias=bias, stats=stats, dy=dy, OH=OH, OW=OW)


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _forward(nat, case, inp, bn):
    """-> (y [NF][OH][OW][Co], the BN partial sums written, flattened)"""
    name, NF, Ci, Co, IH, IW, s = case
    d = torch.device("cuda")
    OH, OW = inp["OH"], inp["OW"]
    y = _nan(NF, OH, OW, Co)
    wf, wd = _nan(9 * Ci * Co), _nan(9 * Ci * Co)
    parts = _nan((NF * OH * OW // 64 + 2) * 2 * Co)
    nparts, cm = np.zeros(1, np.int32), np.ones(1, np.int32)
    x, st, w, b = (inp[k].to(d) for k in ("x", "stats", "w", "bias"))  # (held until the launch has run)
    nat.check(nat.lib().vad_conv3x3_forward_bn(
        x.data_ptr(), st.data_ptr() if bn else None, NF, Ci, IH, IW, w.data_ptr(), b.data_ptr(), Co, s, y.data_ptr(),
        wf.data_ptr(), wd.data_ptr(), parts.data_ptr(), nparts.ctypes.data, cm.ctypes.data, nat.stream_of(d)))
    torch.cuda.synchronize()
    return y.cpu(), parts[:int(nparts[0]) * 2 * Co].cpu()


def _dgrad(nat, case, inp):
    """stride 1: dx and the fused BN-backward partials [2 Ci][nparts]"""
    name, NF, Ci, Co, IH, IW, s = case
    d = torch.device("cuda")
    dx = _nan(NF, IH, IW, Ci)
    wf, wd = _nan(9 * Ci * Co), _nan(9 * Ci * Co)
    parts = _nan(2 * Ci * 512)
    nparts = np.zeros(1, np.int32)
    dy, w, x, st = (inp[k].to(d) for k in ("dy", "w", "x", "stats"))  # (held until the launch has run)
    nat.check(nat.lib().vad_conv3x3_dgrad_bnfuse(
        dy.data_ptr(), NF, Ci, IH, IW, w.data_ptr(), Co, s, dx.data_ptr(), wf.data_ptr(),
        wd.data_ptr(), x.data_ptr(), st.data_ptr(), parts.data_ptr(), parts.numel(),
        nparts.ctypes.data, nat.stream_of(d)))
    torch.cuda.synchronize()
    assert int(nparts[0]) > 0, "the split input gradient fuses the BN-backward reduce"
    return dx.cpu(), parts[:int(nparts[0]) * 2 * Ci].cpu()


def _inputs3d():
    name, N, Ci, Co, D, H, W = CASE3D
    rng = np.random.Generator(np.random.PCG64(sum(map(ord, name))))
    return dict(x=_ints(rng, (N, D, H, W, Ci), 2.0 ** -11), w=_ints(rng, (Co, Ci, 3, 3, 3), 2.0 ** -12 / (27 * Ci) ** 0.5),
                bias=_ints(rng, (Co,), 2.0 ** -12))


def _forward3d(nat, inp):
    name, N, Ci, Co, D, H, W = CASE3D
    d = torch.device("cuda")
    need = nat.lib().vad_conv3d_scratch_floats(0, 3, N, Ci, D, H, W, Co, 1, 1, 1)
    assert need >= 0, nat.lib().vad_last_error()
    sc = _nan(need + 1024)
    y = _nan(N, D, H, W, Co)
    x, w, b = (inp[k].to(d) for k in ("x", "w", "bias"))  # (held until the launch has run)
    nat.check(nat.lib().vad_conv3d_forward(x.data_ptr(), 1, N, Ci, D, H, W, w.data_ptr(), b.data_ptr(), Co, 1, 1, 1, 3,
                                           y.data_ptr(), sc.data_ptr(), sc.numel(), nat.stream_of(d)))
    torch.cuda.synchronize()
    return y.cpu()


_RESULTS = {}


def _results():
    """{case / output: float32 tensor}, computed once for the module."""
    if _RESULTS:
        return _RESULTS
    nat = _lib()
    for case in CASES:
        inp = _inputs(case)
        for bn in (True, False):
            y, parts = _forward(nat, case, inp, bn)
            _RESULTS[f"{case[0]}/fwd_{'bn' if bn else 'raw'}/y"] = y
            _RESULTS[f"{case[0]}/fwd_{'bn' if bn else 'raw'}/parts"] = parts
        if case[-1] == 1:
            dx, parts = _dgrad(nat, case, inp)
            _RESULTS[f"{case[0]}/dgrad/dx"] = dx
            _RESULTS[f"{case[0]}/dgrad/parts"] = parts
    _RESULTS[f"{CASE3D[0]}/fwd_raw/y"] = _forward3d(nat, _inputs3d())
    return _RESULTS


def _digest(t):
    """(SHA-256 of the bytes, wrapping sum of the 32-bit patterns per leading (image, row))"""
    a = np.ascontiguousarray(t.numpy()).view(np.uint32)
    rows = a.reshape(-1, a.shape[-1] * (a.shape[-2] if a.ndim > 2 else 1)) if a.ndim > 1 else a.reshape(1, -1)
    return (np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8).copy(),
            rows.astype(np.uint64).sum(axis=1, dtype=np.uint64))


def record(path=GOLDEN):
    """Writes the golden file from the library now built (run once, on the parent's kernels)."""
    out = {}
    for key, t in _results().items():
        out[key + "/sha"], out[key + "/rows"] = _digest(t)
    np.savez_compressed(path, **out)
    return sorted(out)


def _keys():
    keys = []
    for case in CASES:
        keys += [f"{case[0]}/fwd_bn/y", f"{case[0]}/fwd_bn/parts", f"{case[0]}/fwd_raw/y", f"{case[0]}/fwd_raw/parts"]
        if case[-1] == 1:
            keys += [f"{case[0]}/dgrad/dx", f"{case[0]}/dgrad/parts"]
    return keys + [f"{CASE3D[0]}/fwd_raw/y"]


@pytest.mark.parametrize("key", _keys())
def test_bits_equal_the_parent_commit(key):
    gold = np.load(GOLDEN)
    got = _results()[key]
    sha, rows = _digest(got)
    assert not bool(torch.isnan(got).any()), f"{key}: elements left unwritten (or NaN)"
    assert rows.shape == gold[key + "/rows"].shape, f"{key}: {rows.shape} rows, recorded {gold[key + '/rows'].shape}"
    bad = np.nonzero(rows != gold[key + "/rows"])[0]
    assert bad.size == 0, f"{key}: bits differ from the parent's in {bad.size} (image, row) slices, first {bad[:8]}"
    assert bytes(sha) == bytes(gold[key + "/sha"]), f"{key}: bytes differ from the parent's"


def test_golden_covers_every_output():
    gold = np.load(GOLDEN)
    assert sorted(gold.files) == sorted(k + s for k in _keys() for s in ("/sha", "/rows"))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_bn_on_load_pads_with_zeros(case):
    """Forward with BN + ReLU on load, every shift > 0, against the float64 conv of relu(scale x + shift) zero-padded, by
    the split-accuracy bound of test_kernels_gpu.py (worst error over sum |a||w| below 1e-6 and within 2x that of the
    exact-f32 kernels): a padded tap that became relu(shift) is off by far more."""
    nat = _lib()
    name, NF, Ci, Co, IH, IW, s = case
    inp = _inputs(case)
    sc, sh = inp["stats"][2 * Ci:3 * Ci].double(), inp["stats"][3 * Ci:].double()
    assert bool((sh > 0).all())
    a = torch.relu(inp["x"].double() * sc + sh).permute(0, 3, 1, 2)
    w = inp["w"].double()
    ref = F.conv2d(a, w, inp["bias"].double(), stride=s, padding=1)
    mag = F.conv2d(a.abs(), w.abs(), None, stride=s, padding=1)
    lost = F.conv2d(F.pad(a, (1, 1, 1, 1), value=float(sh.min())), w.abs(), None, stride=s) - mag  # what a lost mask adds
    assert float((lost / mag).max()) > 1e-3
    errs = {}
    try:
        for split in (0, 1):
            nat.lib().vad_set_tuning(b"conv_split", split)
            y = _results()[f"{name}/fwd_bn/y"] if split else _forward(nat, case, inp, True)[0]
            errs[split] = float(((y.permute(0, 3, 1, 2).double() - ref).abs() / mag).max())
    finally:
        nat.lib().vad_set_tuning(b"conv_split", 1)
    print(f"{name}: worst |err| / sum |a||w| split {errs[1]:.3g}, f32 {errs[0]:.3g}")
    assert errs[1] < 1e-6, errs
    assert errs[1] <= 2.0 * errs[0] + 1e-8, errs


def test_kd3_matches_float64():
    name, N, Ci, Co, D, H, W = CASE3D
    inp = _inputs3d()
    x = inp["x"].double().permute(0, 4, 1, 2, 3)
    ref = F.conv3d(x, inp["w"].double(), inp["bias"].double(), padding=1)
    mag = F.conv3d(x.abs(), inp["w"].double().abs(), None, padding=1)
    y = _results()[f"{name}/fwd_raw/y"].permute(0, 4, 1, 2, 3).double()
    assert float(((y - ref).abs() / mag).max()) < 1e-6
