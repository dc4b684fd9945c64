"""Gradient parity of the 3-D clip models and the cad1 autoencoder against a float64 restatement of their step.

The reference-fixture tests (test_ae_gpu / test_a2_gpu / test_mc_gpu) compare with the reference's own float32 CPU
gradients, whose summation order differs from any GPU's, so their gradient tolerances are loose (1e-2 / 2e-3).  Here
the oracle step runs in float64 on the same inputs, parameters and random draws, and every gradient tensor of the
device's first step must match it to relative L2 <= 1e-4 (the cad standard, test_cad_gpu's mask-pinned check), the
golden cases and each model's bench shape alike.  Conv biases that feed a train-mode BatchNorm have an exactly-zero
true gradient: they must stay at rounding-noise level.

cad1 (LeakyReLU(0.1) after every BN and after the decoder's Linear) is compared mask-pinned, like cad: the float64
step takes the device's branch decisions (tests/golden_util.ae_leaky_pins, from the device's raw conv outputs and BN
state).  At its bench shape (B=32, T=16) the unpinned gradients differ by up to 3.7e-3 (encoder.0.weight) although
the forward agrees to 3e-7: a unit within rounding of zero takes the other branch and moves every gradient upstream
of it.  Measured on the float64 oracle itself (tools/r6/ae_grad_diag.py, profiles/r06_ae_grad_pinning.json): 1e-7
relative noise on the decoder's ConvTranspose2d outputs moves encoder.0's gradient by 2.2e-4 with the branches free
and by 1.4e-7 with them pinned.  a2 and minicausal need no pinning on these cases (unpinned <= 6e-6).

minicausal's classifier.6.bias is the exception the float64 oracle exposes: its gradient is a mean of (o - y) over
alternating labels with o ~ 0.5, so ANY float32 evaluation misses the exact value by ~1e-3 of it (the torch CPU
restatement: 1.2e-3).  There the bound is derived, not chosen: the float32 restatement is measured against float64
on the same case, and the device must lie within 2x its distance (and within 1e-4 where that distance is below it).
"""
import numpy as np
import pytest
import torch

from oracle import a2_oracle as ao
from oracle import ae_oracle as ae
from oracle import mc_oracle as mo
from tests.golden.cases import A2_CASES, AE_CASES, MC_CASES
from tests.golden_util import ae_case_data, ae_leaky_pins, ae_memory_init
from tests.test_a2_oracle import make_a2_model
from tests.test_ae_oracle import PRE_BN_BIASES as AE_PRE_BN
from tests.test_ae_oracle import make_ae_model
from tests.test_mc_oracle import make_mc_model, split_state

pytestmark = pytest.mark.gpu
MC_PRE_BN = ("features.0.bias", "features.4.bias", "features.8.bias")
TOL = 1e-4


def _rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


def _d64(d):
    return {k: v.detach().double().clone() for k, v in d.items()}


def _device_slots(e):
    return {name: g.cpu().numpy().astype(np.float64) for name, g in e.grad_dict().items()}


def _check(dev, ref, pre_bn, label, bound=None):
    worst, bad = [], []
    for name, r in ref.items():
        d = dev[name]
        r = r.reshape(-1).numpy()
        if name in pre_bn:
            wn = float(np.linalg.norm(ref[name[:-4] + "weight"].numpy()))
            if not float(np.abs(d).max()) <= 1e-5 * wn + 1e-9:
                bad.append(f"{name}: pre-BN bias grad {float(np.abs(d).max()):.3g} above noise")
            continue
        rel = _rel(d, r)
        lim = TOL if bound is None else bound[name]
        worst.append((rel, lim, name))
        if not rel <= lim:
            bad.append(f"{name}: rel-L2 {rel:.3g} > {lim:.3g}")
    worst.sort(reverse=True)
    print(label, " ".join(f"{n}={r:.2e}/{l:.1e}" for r, l, n in worst[:6]))
    assert not bad, f"{label}: " + "; ".join(bad)


# ------------------------------------------------------------------------------------------------- cad1 autoencoder
AE_BENCH = dict(name="bench_b32t16", B=32, T=16, seed=50, lr=1e-5, labels=[[0] * 32], val_labels=[0],
                test_labels=[0], mem=(20, 20))


@pytest.mark.parametrize("case", AE_CASES + [AE_BENCH], ids=[c["name"] for c in AE_CASES] + ["bench_b32t16"])
def test_ae_first_step_grads_match_float64(case):
    ae_step_vs_float64(case)


def ae_step_vs_float64(case):
    """cad1's first train step on the device vs the float64 step pinned to the device's LeakyReLU decisions."""
    from vad_amd.ae import AeTrainer
    model = make_ae_model(case)
    params, bufs, _ = ae.split_state(model.state_dict())
    mem, ptr = ae_memory_init(case)
    train, _, _ = ae_case_data(case)
    v = next(x[y == 0] for x, y in train if bool((y == 0).any()))
    model = model.cuda()
    tr = AeTrainer(model, lr=case["lr"])
    l = tr.step(v.cuda()).cpu().numpy()
    assert int(l[3]) == 2
    e = model.engine()
    dev = _device_slots(e)
    B, T = v.shape[0], v.shape[1]
    pins = ae_leaky_pins(e.plans[(B, T)], B, T)
    leaves = {n: t.requires_grad_(True) for n, t in _d64(params).items()}
    out = ae.ae_forward(leaves, _d64(bufs), v.double(), True, mem.double(), ptr, pins=pins)
    loss = ae.safe_mse(out["reconstructed"], v.double())
    assert float(l[0]) == pytest.approx(float(loss), rel=1e-5)
    loss.backward()
    _check(dev, {n: t.grad for n, t in leaves.items()}, AE_PRE_BN, f"ae/{case['name']}")


# ---------------------------------------------------------------------------------------------------------------- a2
A2_BENCH = dict(name="bench_b32t8", B=32, T=8, H=64, W=64, seed=60, step=0, ckpt=False)


@pytest.mark.parametrize("case", A2_CASES + [A2_BENCH], ids=[c["name"] for c in A2_CASES] + ["bench_b32t8"])
def test_a2_first_step_grads_match_float64(case):
    from vad_amd.a2 import ImprovedMiniCausalVAD
    B, T, H, W = case["B"], case["T"], case["H"], case["W"]
    model = make_a2_model(case)
    params = {k: v.clone() for k, v in model.state_dict().items()}
    vad = ImprovedMiniCausalVAD(device="cuda")
    vad.model = model.to("cuda")
    vad.seed, vad.global_step, vad.clip0 = case["seed"], case["step"], 0
    x = ao.synth_clips(case["seed"], case["step"], 0, B, T, H, W)
    avg, _ = vad.train_epoch_improved([(x, ao.synth_labels(0, B))])
    dev = _device_slots(vad.model._engine)
    leaves = {n: t.requires_grad_(True) for n, t in _d64(params).items()}
    draws = ao.A2Draws.make(case["seed"], case["step"], 0, B)
    s, adj, _ = ao.a2_forward(leaves, x.double(), draws, True)
    total, _, _ = ao.a2_loss(s, adj, draws.u_pseudo)
    assert avg == pytest.approx(float(total), rel=1e-5)
    total.backward()
    _check(dev, {n: t.grad for n, t in leaves.items()}, (), f"a2/{case['name']}")


# -------------------------------------------------------------------------------------------------------- minicausal
MC_BENCH = dict(name="bench_b32t16_64", B=32, T=16, H=64, W=64, seed=13, step=0, scale=1.0)


def _mc_oracle_grads(params, bufs, x, y, draws, dtype):
    leaves = {n: t.detach().to(dtype).clone().requires_grad_(True) for n, t in params.items()}
    b = {k: v.detach().to(dtype).clone() for k, v in bufs.items()}
    o = mo.mc_forward(leaves, b, x.to(dtype), draws, True).squeeze()
    loss = torch.nn.functional.binary_cross_entropy(o, y.to(dtype))
    loss.backward()
    return float(loss), {n: t.grad.double() for n, t in leaves.items()}


@pytest.mark.parametrize("case", MC_CASES + [MC_BENCH], ids=[c["name"] for c in MC_CASES] + ["bench_b32t16_64"])
def test_mc_first_step_grads_match_float64(case):
    from vad_amd.mc import StableTrainer
    B, T, H, W = case["B"], case["T"], case["H"], case["W"]
    model = make_mc_model(case)
    params, bufs = split_state(model)
    x = mo.synth_clips(case["seed"], case["step"], 0, B, T, H, W)
    y = mo.synth_labels(0, B)
    tr = StableTrainer(model, [(x, y)], [], "cuda", lr=1e-3)
    tr.seed, tr.global_step, tr.clip0 = case["seed"], case["step"], 0
    tr.train_epoch()
    dev = _device_slots(model._engine)
    draws = mo.McDraws.make(case["seed"], case["step"], 0, B)
    l64, g64 = _mc_oracle_grads(params, bufs, x, y, draws, torch.float64)
    _, g32 = _mc_oracle_grads(params, bufs, x, y, draws, torch.float32)
    assert float(model._engine.losses[0]) == pytest.approx(l64, rel=1e-5)
    # derived bound per tensor: 2x the float32 restatement's own distance from float64, at least TOL
    bound = {n: max(TOL, 2.0 * _rel(g32[n].numpy(), g64[n].numpy())) for n in g64}
    _check(dev, g64, MC_PRE_BN, f"mc/{case['name']}", bound)
