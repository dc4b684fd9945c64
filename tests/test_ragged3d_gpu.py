"""The three 3-D clip models at ragged shapes against their float64 oracles: odd T / H / W into the stride-2 convs (a2),
MaxPool3d windows that do not divide their extent and partial direct-conv tiles (minicausal), odd extents under the
fused conv + MaxPool3d(2) stem (bbox) -- on the default kernels and on the im2col + GEMM path of each plan.

Tolerances are those of tests/test_grad64.py (whose helpers are reused): relative L2 <= 1e-4 per gradient tensor for
a2 (the float32 CPU oracle itself lies within 6.1e-7 of float64 on every tensor at these four shapes); for minicausal
the bound derived there, 2x the float32 oracle's own distance from float64 with a floor of 1e-4 (<= 4.2e-6 on every
tensor but classifier.6.bias, whose gradient cancels to 3e-5 .. 6e-3 at B = 2); bbox: rtol 1e-4 with the atols of
test_bbox_hip_matches_reference.  No shape needs its ReLU decisions pinned."""
import functools

import numpy as np
import pytest
import torch

from oracle import a2_oracle as ao
from oracle import bbox_oracle as bo
from oracle import mc_oracle as mo
from tests.test_a2_oracle import make_a2_model
from tests.test_bbox import make_bbox_model
from tests.test_grad64 import MC_PRE_BN, TOL, _check, _d64, _device_slots, _mc_oracle_grads, _rel
from tests.test_mc_oracle import make_mc_model, split_state

pytestmark = pytest.mark.gpu


class _knobs:
    """library tuning knobs for the duration of a block; their defaults restored on the way out"""
    DEFAULTS = {b"a2_direct": 1, b"conv3d_direct": 1, b"maxpool3d_bwd_win": 1, b"bbox_im2col": 0}

    def __init__(self, **kv):
        self.kv = {k.encode(): v for k, v in kv.items()}

    def __enter__(self):
        from vad_amd import _native as nat
        for k, v in self.kv.items():
            nat.check(nat.lib().vad_set_tuning(k, v))

    def __exit__(self, *exc):
        from vad_amd import _native as nat
        for k in self.kv:
            nat.check(nat.lib().vad_set_tuning(k, self.DEFAULTS[k]))


# ---------------------------------------------------------------------------------------------------------------- a2
A2_RAGGED = [dict(name=f"b{B}t{T}_{H}x{W}", B=B, T=T, H=H, W=W, seed=70 + i, step=0, ckpt=False)
             for i, (B, T, H, W) in enumerate([(3, 5, 37, 27), (2, 7, 50, 46), (2, 1, 9, 9), (2, 3, 4, 5)])]


@functools.lru_cache(maxsize=None)
def _a2_oracle(name):
    case = next(c for c in A2_RAGGED if c["name"] == name)
    B, T, H, W = case["B"], case["T"], case["H"], case["W"]
    params = {k: v.clone() for k, v in make_a2_model(case).state_dict().items()}
    x = ao.synth_clips(case["seed"], case["step"], 0, B, T, H, W)
    leaves = {n: t.requires_grad_(True) for n, t in _d64(params).items()}
    draws = ao.A2Draws.make(case["seed"], case["step"], 0, B)
    s, adj, _ = ao.a2_forward(leaves, x.double(), draws, True)
    total, _, _ = ao.a2_loss(s, adj, draws.u_pseudo)
    total.backward()
    return float(total), {n: t.grad for n, t in leaves.items()}


@pytest.mark.parametrize("direct", [1, 0], ids=["direct", "im2col"])
@pytest.mark.parametrize("case", A2_RAGGED, ids=[c["name"] for c in A2_RAGGED])
def test_a2_ragged_first_step_grads_match_float64(case, direct):
    """a2's first train step at odd extents: 37 -> 19 -> 10 -> 5, 27 -> 14 -> 7 -> 4, T = 5 -> 3 -> 2, a single frame,
    and a 4 x 5 frame whose last conv sees one voxel (every adaptive-average bin reads it).  The a2_direct knob is
    latched when the plan is created, so each run builds a fresh model under it."""
    from vad_amd.a2 import ImprovedMiniCausalVAD
    B, T, H, W = case["B"], case["T"], case["H"], case["W"]
    total, ref = _a2_oracle(case["name"])
    with _knobs(a2_direct=direct):
        vad = ImprovedMiniCausalVAD(device="cuda")
        vad.model = make_a2_model(case).to("cuda")
        vad.seed, vad.global_step, vad.clip0 = case["seed"], case["step"], 0
        x = ao.synth_clips(case["seed"], case["step"], 0, B, T, H, W)
        avg, _ = vad.train_epoch_improved([(x, ao.synth_labels(0, B))])
        dev = _device_slots(vad.model._engine)
    assert avg == pytest.approx(total, rel=1e-5)
    _check(dev, ref, (), f"a2/{case['name']}/direct{direct}")


# -------------------------------------------------------------------------------------------------------- minicausal
# B odd except at the smallest shape the plan accepts
MC_RAGGED = [dict(name=f"b{B}t{T}_{H}x{W}", B=B, T=T, H=H, W=W, seed=80 + i, step=0, scale=1.0)
             for i, (B, T, H, W) in enumerate([(3, 5, 19, 27), (3, 9, 33, 17), (2, 4, 8, 8)])]


def _mc_inputs(case):
    x = mo.synth_clips(case["seed"], case["step"], 0, case["B"], case["T"], case["H"], case["W"])
    return x, mo.synth_labels(0, case["B"])


@functools.lru_cache(maxsize=None)
def _mc_oracle(name):
    case = next(c for c in MC_RAGGED if c["name"] == name)
    params, bufs = split_state(make_mc_model(case))
    x, y = _mc_inputs(case)
    draws = mo.McDraws.make(case["seed"], case["step"], 0, case["B"])
    l64, g64 = _mc_oracle_grads(params, bufs, x, y, draws, torch.float64)
    _, g32 = _mc_oracle_grads(params, bufs, x, y, draws, torch.float32)
    # derived bound per tensor: 2x the float32 restatement's own distance from float64, at least TOL
    return l64, g64, {n: max(TOL, 2.0 * _rel(g32[n].numpy(), g64[n].numpy())) for n in g64}


@functools.lru_cache(maxsize=None)
def _mc_device(name, direct, win):
    """one device train step under the two knobs (a fresh model: the plan sizes its buffers by conv3d_direct):
    loss, gradient slots, post-step parameters"""
    from vad_amd.mc import StableTrainer
    case = next(c for c in MC_RAGGED if c["name"] == name)
    with _knobs(conv3d_direct=direct, maxpool3d_bwd_win=win):
        model = make_mc_model(case)
        x, y = _mc_inputs(case)
        tr = StableTrainer(model, [(x, y)], [], "cuda", lr=1e-3)
        tr.seed, tr.global_step, tr.clip0 = case["seed"], case["step"], 0
        tr.train_epoch()
        return (float(model._engine.losses[0]), _device_slots(model._engine),
                torch.cat([p.detach().reshape(-1).cpu() for p in model.parameters()]))


@pytest.mark.parametrize("win", [1, 0], ids=["poolwin", "poolelem"])
@pytest.mark.parametrize("direct", [1, 0], ids=["direct", "im2col"])
@pytest.mark.parametrize("case", MC_RAGGED, ids=[c["name"] for c in MC_RAGGED])
def test_mc_ragged_first_step_grads_match_float64(case, direct, win):
    """minicausal's first step where no pooling window divides its extent (19 / 2, 9 / 2, 27 / 2, T = 5 and 9 under the
    (2, 2, 2) pools: the window backward clears the remainder first), the 2-deep direct-conv tile is partial in D, and
    at the smallest shape the plan accepts (T = 4, 8 x 8: the last pool leaves one voxel)."""
    l64, g64, bound = _mc_oracle(case["name"])
    loss, dev, _ = _mc_device(case["name"], direct, win)
    assert loss == pytest.approx(l64, rel=1e-5)
    _check(dev, g64, MC_PRE_BN, f"mc/{case['name']}/direct{direct}/win{win}", bound)


@pytest.mark.parametrize("direct", [1, 0], ids=["direct", "im2col"])
def test_mc_ragged_pool_backward_kernels_are_bit_identical(direct):
    """Both MaxPool3d backward kernels leave bit-identical parameters after the step at a shape whose windows do not
    cover the volume (the window kernel's cleared remainder equals the element kernel's zeros)."""
    name = MC_RAGGED[0]["name"]
    assert torch.equal(_mc_device(name, direct, 1)[2], _mc_device(name, direct, 0)[2])


# -------------------------------------------------------------------------------------------------------------- bbox
BBOX_RAGGED = [(2, 7, 37, 45), (1, 2, 2, 2), (3, 9, 33, 17), (2, 5, 9, 7)]


@functools.lru_cache(maxsize=None)
def _bbox_oracle(shape):
    p = {k: v.detach().double() for k, v in make_bbox_model(dict(seed=90)).state_dict().items()}
    x = bo.synth_clips(91, 0, 0, *shape)
    with torch.no_grad():
        s, adj, f = bo.bbox_forward(p, x.double())
    return x, s.reshape(-1).numpy(), adj.numpy(), f.numpy()


@pytest.mark.parametrize("im2col", [0, 1], ids=["fused", "im2col"])
@pytest.mark.parametrize("shape", BBOX_RAGGED, ids=["b{}t{}_{}x{}".format(*s) for s in BBOX_RAGGED])
def test_bbox_ragged_forward_matches_float64(shape, im2col):
    """bbox eval forward where the fused conv + MaxPool3d(2) stem drops the last slice, row and column (odd T, H, W),
    down to the 2 x 2 x 2 clip that pools to one voxel: scores, adjacency and features against float64."""
    x, rs, radj, rf = _bbox_oracle(shape)
    m = make_bbox_model(dict(seed=90)).cuda()
    with _knobs(bbox_im2col=im2col), torch.no_grad():
        s, adj, f = [t.cpu().double().numpy() for t in m(x.cuda())]
    np.testing.assert_allclose(s.reshape(-1), rs, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(adj.reshape(radj.shape), radj, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(f.reshape(rf.shape), rf, rtol=1e-4, atol=1e-5)
