"""HIP train step of CausalAnomalyDetector against the reference's golden vectors and the CPU oracle.

Tolerances: scores/losses 1e-4 (north star).  Gradients: the ReLU after every train-mode BatchNorm makes the
gradient discontinuous at BN outputs == 0, and an element within one rounding of 0 can take the other branch in
any re-implementation (the reference's own fp32 run included), which moves one output channel of the conv weight
grad below it by a few % of its RMS.  The gradients are therefore pinned against the *mask-pinned* oracle: a
float64 oracle backward that takes the ReLU decisions of the HIP forward (tests/golden_util.hip_relu_masks), i.e.
the exact gradient of the branch the device took.  Every gradient tensor must match it to relative L2 <= 1e-4 (the
conv biases in front of a BatchNorm, whose true gradient is exactly 0, to rounding noise).  The oracle itself is
pinned to the reference by tests/test_oracle_golden.py.  Post-step parameters: equal (fp32 rounding) to
torch.optim.AdamW applied in float64 to the device's own clipped gradients, and to the reference's post-step
samples on the small cases."""
import numpy as np
import pytest
import torch

from oracle import cad_oracle as co
from tests.golden_util import (BF16_SPREAD, cad_cases, check_mask_flips, hip_relu_masks, load,  # noqa: F401
                               make_cad_model, pinned_oracle_grads, rel_l2)
from tests.test_oracle_golden import is_pre_bn_bias

pytestmark = pytest.mark.gpu
CASES = cad_cases()


def _frozen(m):
    from vad_amd.train import apply_memory_efficient_training
    import io, contextlib
    with contextlib.redirect_stdout(io.StringIO()):
        apply_memory_efficient_training(m)
    return m


def _module_pinned_check(m, case, x, user_loss, training, seed=0, step=0, coef=None):
    """model(x) + user_loss(out).backward() on the device against the mask-pinned float64 oracle (the eight conv ReLUs,
    bn1's ReLU and the MaxPool2d window maxima taken from the HIP forward): scores / probabilities within 1e-4 and
    every parameter gradient within relative L2 1e-4 per tensor (train mode: the pre-BN conv biases, true gradient 0,
    at rounding noise; eval mode normalises with running statistics, so they carry a real gradient there).
    Returns (worst relative L2, names of the tensors with a live gradient, the oracle's output)."""
    from tests.golden_util import hip_stem_pins, reshape_masks
    B, T, H, W = x.shape[0], x.shape[1], x.shape[3], x.shape[4]
    out = m(x.cuda(), seed=seed, step=step, clip0=0) if training else m(x.cuda())
    user_loss(out, coef.cuda() if coef is not None else None).backward()
    torch.cuda.synchronize()
    eng = m.engine()
    masks = reshape_masks(hip_relu_masks(eng, B * T), x)
    pins = hip_stem_pins(eng, B * T, H, W) if eng.stem_grad_on else None
    sd = make_cad_model(case).state_dict()
    params = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items()
              if "running" not in k and "num_batches" not in k}
    bufs = {k: v.detach().double().clone() for k, v in sd.items() if "running" in k}
    ref = co.cad_forward(params, bufs, x.double(), co.CadDraws.make(seed, step, 0, B, T), training=training,
                         relu_masks=masks, stem_pins=pins)
    user_loss(ref, coef.double() if coef is not None else None).backward()
    np.testing.assert_allclose(out["anomaly_scores"].detach().cpu().numpy(), ref["anomaly_scores"].detach().numpy(),
                               rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(out["direct_predictions"].detach().cpu().numpy(),
                               ref["direct_predictions"].detach().numpy(), rtol=1e-4, atol=1e-5)
    worst, live = 0.0, set()
    for n, p in m.named_parameters():
        pr = params[n]
        if pr.grad is None or float(pr.grad.abs().max()) == 0.0:
            assert p.grad is None or float(p.grad.abs().max()) < 1e-9, n
            continue
        assert p.grad is not None, n
        mine = p.grad.detach().cpu().double().numpy()
        if training and (is_pre_bn_bias(n) or n == "backbone.conv1.bias"):  # true gradient 0 (BN removes the mean)
            assert np.abs(mine).max() < 1e-6 * max(1.0, float(pr.grad.abs().max())) + 1e-6, n
            continue
        e = rel_l2(mine, pr.grad.numpy())
        worst = max(worst, e)
        live.add(n)
        assert e <= 1e-4, f"{n}: relative L2 error {e:.3g} vs the mask-pinned oracle"
    return worst, live, ref


def _hip_step(case, step_opt=True, keep_pre=False):
    from vad_amd.train import apply_memory_efficient_training
    import io, contextlib
    m = make_cad_model(case)
    with contextlib.redirect_stdout(io.StringIO()):
        apply_memory_efficient_training(m)
    m = m.cuda()
    eng = m.engine()
    B, T, H, W = case["B"], case["T"], case["H"], case["W"]
    x = co.synth_clips(case["seed"], case["step"], 0, B, T, H, W).cuda()
    y = co.synth_labels(0, B).cuda()
    pre = eng.params.clone() if keep_pre else None
    o = eng.forward(x, True, case["seed"], case["step"], 0, y)
    eng.backward(True)
    torch.cuda.synchronize()
    grads = eng.grads.clone()
    masks = hip_relu_masks(eng, B * T) if keep_pre else None
    tn = torch.zeros(1, device="cuda")
    if step_opt:
        eng.optimizer_step(3e-4, total_norm=tn)
    torch.cuda.synchronize()
    if keep_pre:
        return m, eng, o, grads, tn, pre, masks
    return m, eng, o, grads, tn


def check_pinned_grads(eng, gr, ref_grads, tol=1e-4):
    """Every live gradient tensor vs the mask-pinned float64 oracle (relative L2); conv biases in front of a
    BatchNorm (true gradient 0) at rounding noise.  Returns the worst relative error."""
    worst = 0.0
    for i, n in enumerate(eng.slot_names):
        ref = ref_grads.get(n)
        mine = gr[eng.slot_offset[i]:eng.slot_offset[i] + eng.slot_numel[i]].astype(np.float64)
        if ref is None:
            assert np.abs(mine).max() == 0.0, n
            continue
        if is_pre_bn_bias(n):
            assert np.abs(mine).max() < 1e-6, n
            continue
        e = rel_l2(mine, ref.detach().numpy())
        worst = max(worst, e)
        assert e <= tol, f"{n}: relative L2 error {e:.3g} vs the mask-pinned oracle"
    return worst


def check_adamw_applied(eng, pre, gr, post, tn, lr=3e-4, wd=1e-5, max_norm=1.0):
    """Post-step params == torch AdamW (first step) applied in float64 to the device's clipped grads."""
    p = pre.double().cpu().numpy()
    g = gr[:eng.param_floats].astype(np.float64)
    flags = gr[eng.param_floats:eng.param_floats + 2]
    norm = float(np.sqrt((g * g).sum()))
    assert float(tn) == pytest.approx(norm, rel=1e-5)
    coef = min(1.0, max_norm / (norm + 1e-6))
    want = p.copy()
    for i, grp in enumerate(eng.slot_group):
        if not (grp == 1 or (grp == 2 and flags[0] > 0) or (grp == 3 and flags[1] > 0)):
            continue
        o, k = eng.slot_offset[i], eng.slot_numel[i]
        gi = g[o:o + k] * coef
        m = 0.1 * gi
        v = 0.001 * gi * gi
        want[o:o + k] = p[o:o + k] * (1 - lr * wd) - (lr / 0.1) * m / (np.sqrt(v) / np.sqrt(0.001) + 1e-8)
    got = post.double().cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=2e-7, atol=1e-9)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hip_step_matches_reference(case):
    g = load(f"cad_{case['name']}.npz")
    m, eng, o, grads, tn, pre, masks = _hip_step(case, keep_pre=True)
    tol = dict(rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(o["final"].cpu().numpy(), g["out/anomaly_scores"], **tol)
    np.testing.assert_allclose(o["probs"].cpu().numpy(), g["out/direct_predictions"], **tol)
    np.testing.assert_allclose(o["causal"].cpu().numpy(), g["out/causal_anomaly_scores"], **tol)
    np.testing.assert_allclose(o["kl"].cpu().numpy(), g["out/kl"], **tol)
    np.testing.assert_array_equal(o["nmax"].cpu().numpy(), g["out/nmax"])
    np.testing.assert_array_equal(o["counts"].cpu().numpy(), g["out/det_count"])
    np.testing.assert_allclose(o["z"].cpu().numpy(), g["out/z"], **tol)
    np.testing.assert_allclose(o["adj"].cpu().numpy(), g["out/adj"], **tol)
    np.testing.assert_allclose(o["boxes"].cpu().numpy(), g["out/det_boxes"], rtol=1e-4, atol=1e-3)
    losses = o["losses"].cpu().numpy()
    for i, k in enumerate(("classification", "anomaly", "causal", "kl", "total")):
        assert losses[i] == pytest.approx(float(g[f"loss/{k}"]), rel=1e-4, abs=1e-6), k
    assert float(tn.item()) == pytest.approx(float(g["grad_total_norm"]), rel=1e-3)
    gr = grads.cpu().numpy()
    flags = gr[eng.param_floats:eng.param_floats + 2]
    for i, n in enumerate(eng.slot_names):
        grp = eng.slot_group[i]
        has = int(g[f"has_grad/{n}"]) if f"has_grad/{n}" in g else 0
        live = grp == 1 or (grp == 2 and flags[0] > 0) or (grp == 3 and flags[1] > 0)
        assert int(live) == has, n
    # gradients: every tensor against the mask-pinned float64 oracle
    B, T, H, W = case["B"], case["T"], case["H"], case["W"]
    sd = make_cad_model(case).state_dict()
    x = co.synth_clips(case["seed"], case["step"], 0, B, T, H, W)
    ref_grads, ref_losses, _ = pinned_oracle_grads(sd, x, co.synth_labels(0, B),
                                                   co.CadDraws.make(case["seed"], case["step"], 0, B, T), masks)
    check_pinned_grads(eng, gr, ref_grads)
    # and the golden's own samples on the small cases (no ReLU-kink element there: checked element-wise)
    if case["H"] * case["W"] <= 100 * 100:
        for i, n in enumerate(eng.slot_names):
            if f"idx/{n}" not in g or is_pre_bn_bias(n) or not int(g.get(f"has_grad/{n}", 0)):
                continue
            off, nel = eng.slot_offset[i], eng.slot_numel[i]
            gf = gr[off:off + nel]
            ref_norm = float(g[f"grad_norm/{n}"])
            assert float(np.linalg.norm(gf.astype(np.float64))) == pytest.approx(ref_norm, rel=2e-3, abs=1e-9), n
    # post-step parameters: AdamW on the device's own grads, exactly
    check_adamw_applied(eng, pre, gr, eng.params, tn.item())
    sd = m.state_dict()
    for n, t in sd.items():
        if "num_batches" in n:
            assert int(t.item()) == 1, n
            continue
        if case["H"] * case["W"] > 100 * 100 and "running" not in n:
            continue  # large cases: post-step params are pinned through the grads (above)
        tf = t.detach().cpu().numpy().reshape(-1)
        atol = 3.01e-4 if is_pre_bn_bias(n) else 1.5e-5
        np.testing.assert_allclose(tf[g[f"idx/{n}"]], g[f"post/{n}"], rtol=1e-5, atol=atol, err_msg=n)


def test_module_api_forward_backward():
    """model(videos) through torch autograd in eval mode (running statistics; the stem trains: no freeze): output
    structure, and the scores plus every gradient of a user-defined loss vs the mask-pinned float64 oracle (relative
    L2 <= 1e-4 per tensor)."""
    case = dict(name="api", B=2, T=4, H=64, W=64, seed=11, step=0, forced=None)
    m = make_cad_model(case).cuda()
    m.eval()
    x = co.synth_clips(11, 0, 0, 2, 4, 64, 64)
    out = m(x.cuda())
    assert set(out) == {"anomaly_scores", "causal_factors", "adjacency_matrices", "kl_losses", "detections",
                        "direct_predictions", "causal_anomaly_scores"}
    assert len(out["detections"]) == 2 and len(out["detections"][0]) == 4

    def user_loss(o, _):
        return o["anomaly_scores"].sum() + 0.5 * o["direct_predictions"][:, 0].sum() + sum(o["kl_losses"])

    m.zero_grad(set_to_none=True)
    worst, live, _ = _module_pinned_check(m, case, x, user_loss, training=False)
    assert any(n.startswith("backbone.conv1.") for n in live)  # (the stem trains: the reference module unfrozen)
    print(f"worst per-tensor relative L2 vs the mask-pinned oracle: {worst:.3g}")


@pytest.mark.parametrize("B,T,H,W", [(8, 16, 227, 227)])
def test_hip_forward_matches_oracle_full_size(B, T, H, W):
    """Config-2 shape (B=8, T=16, 227x227): forward scores and losses vs the CPU oracle."""
    case = dict(name="cfg2", B=B, T=T, H=H, W=W, seed=5, step=2, forced=None)
    m = make_cad_model(case).cuda()
    eng = m.engine()
    x = co.synth_clips(5, 2, 0, B, T, H, W)
    y = co.synth_labels(0, B)
    o = eng.forward(x.cuda(), True, 5, 2, 0, y.cuda())
    mc = make_cad_model(case)
    sd = {k: v.clone() for k, v in mc.state_dict().items()}
    params = {k: v for k, v in sd.items() if "running" not in k and "num_batches" not in k}
    bufs = {k: v for k, v in sd.items() if "running" in k}
    with torch.no_grad():
        ref = co.cad_forward(params, bufs, x, co.CadDraws.make(5, 2, 0, B, T), training=True)
        rl = co.cad_losses(ref, y)
    np.testing.assert_allclose(o["final"].cpu().numpy(), ref["anomaly_scores"].numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(o["probs"].cpu().numpy(), ref["direct_predictions"].numpy(), rtol=1e-4, atol=1e-5)
    assert float(o["losses"][4]) == pytest.approx(float(rl["total"]), rel=1e-4)
    for k in bufs:
        np.testing.assert_allclose(dict(m.named_buffers())[k].cpu().numpy(), bufs[k].numpy(), rtol=1e-4, atol=1e-4,
                                   err_msg=k)


def test_hip_backward_matches_oracle_full_size():
    """Config-2 shape (B=8, T=16, 227x227): every gradient tensor vs the mask-pinned float64 oracle, relative L2
    <= 1e-4, and the loss terms within 1e-4."""
    B, T, H, W = 8, 16, 227, 227
    case = dict(name="cfg2", B=B, T=T, H=H, W=W, seed=6, step=0, forced=None)
    m = _frozen(make_cad_model(case)).cuda()  # train_model's frozen stem (cad:592-598), as the oracle step
    eng = m.engine()
    x = co.synth_clips(6, 0, 0, B, T, H, W)
    y = co.synth_labels(0, B)
    o = eng.forward(x.cuda(), True, 6, 0, 0, y.cuda())
    eng.backward(True)
    torch.cuda.synchronize()
    gr = eng.grads.cpu().numpy()
    masks = hip_relu_masks(eng, B * T)
    ref_grads, ref_losses, res = pinned_oracle_grads(make_cad_model(case).state_dict(), x, y,
                                                     co.CadDraws.make(6, 0, 0, B, T), masks)
    assert float(o["losses"][4]) == pytest.approx(float(ref_losses["total"]), rel=1e-4)
    worst = check_pinned_grads(eng, gr, ref_grads)
    flips = check_mask_flips(masks, res["record"], x)
    print(f"worst per-tensor relative L2 vs the mask-pinned oracle: {worst:.3g}; ReLU decisions that differ from "
          f"the float64 forward per layer (count, worst |z| / bound): {flips}")


@pytest.mark.parametrize("B,T,H,W", [(2, 8, 227, 227), (1, 4, 256, 256), (1, 3, 64, 80)])
def test_fused_stem_matches_float64_stem(B, T, H, W):
    """Frozen stem (stem.hip: conv1 + BN sums + 3x3/s2 pooling of the raw output -- max where gamma >= 0, min where
    gamma < 0 -- in one pass, bn1 + ReLU applied on load by layer1.0) against the float64 stem
    maxpool(relu(bn1_train(conv1(x)))) and against the stored-activation path (knob stem_fused=0); bn1's running
    statistics too.  One bn1 gamma is made negative so both pooling directions are exercised."""
    from tests.golden_util import read_debug
    from vad_amd import _native as nat
    case = dict(name="stem", B=B, T=T, H=H, W=W, seed=9, step=1, forced=None)
    x = co.synth_clips(9, 1, 0, B, T, H, W)
    y = co.synth_labels(0, B)
    pools, rstats = [], []
    for fused in (1, 0):
        nat.check(nat.lib().vad_set_tuning(b"stem_fused", fused))
        try:
            m = _frozen(make_cad_model(case))
            with torch.no_grad():
                m.backbone.bn1.weight[3] = -0.75
            m = m.cuda()
            eng = m.engine()
            eng.forward(x.cuda(), True, 9, 1, 0, y.cuda())
            torch.cuda.synchronize()
            pool = read_debug(eng._last[0], "pool").astype(np.float64)
            if fused:  # raw pooled conv1 output: bn1 + ReLU as layer1.0 applies them on load
                st = read_debug(eng._last[0], "stats", 0).astype(np.float64)
                pool = np.maximum(pool.reshape(-1, 32) * st[64:96] + st[96:128], 0.0).reshape(-1)
            pools.append(pool)
            bufs = dict(m.named_buffers())
            rstats.append([bufs[k].cpu().numpy() for k in ("backbone.bn1.running_mean", "backbone.bn1.running_var")])
        finally:
            nat.check(nat.lib().vad_set_tuning(b"stem_fused", 1))
    sd = make_cad_model(case).state_dict()
    sd["backbone.bn1.weight"] = sd["backbone.bn1.weight"].clone()
    sd["backbone.bn1.weight"][3] = -0.75
    xd = x.reshape(B * T, 1, H, W).double()
    c = torch.nn.functional.conv2d(xd, sd["backbone.conv1.weight"].double(), sd["backbone.conv1.bias"].double(),
                                   stride=2, padding=3)
    mean, var = c.mean(dim=(0, 2, 3)), c.var(dim=(0, 2, 3), unbiased=False)
    z = (c - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + 1e-5)
    z = z * sd["backbone.bn1.weight"].double()[None, :, None, None] + sd["backbone.bn1.bias"].double()[None, :, None, None]
    ref = torch.nn.functional.max_pool2d(torch.relu(z), 3, 2, 1).permute(0, 2, 3, 1).reshape(-1).numpy()
    scale = float(np.abs(ref).max())
    for got in pools:
        assert got.shape == ref.shape
        np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5 * scale)
    np.testing.assert_allclose(pools[0], pools[1], rtol=1e-5, atol=1e-6 * scale)
    rm = 0.9 * sd["backbone.bn1.running_mean"].double() + 0.1 * mean
    rv = 0.9 * sd["backbone.bn1.running_var"].double() + 0.1 * c.var(dim=(0, 2, 3), unbiased=True)
    for got_m, got_v in rstats:
        np.testing.assert_allclose(got_m, rm.numpy(), rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(got_v, rv.numpy(), rtol=1e-5, atol=1e-7)


def test_module_api_train_mode_unfrozen_227():
    """The module API in train mode WITHOUT the trainer's freeze (the reference's CausalAnomalyDetector used as a
    plain nn.Module: conv1 / bn1 train with batch statistics, cad:115-116,145-147; the freeze is only in train_model,
    cad:592-598), forced detections (live boxes: detector and detection-box grads), B=2, T=16, 227x227:
    model.train(); out = model(x); loss.backward() for a user loss over scores, probabilities, KL terms and the
    detections.  Every parameter gradient vs the mask-pinned float64 oracle (the eight conv ReLUs, bn1's ReLU and
    the MaxPool2d window maxima taken from the HIP forward) to relative L2 <= 1e-4 per tensor -- this covers bn1's
    batch-statistics backward, maxpool_bwd, conv1's weight gradient and the detection-box grads in train mode; the
    scores within 1e-4 and bn1's running statistics too."""
    from tests.golden.cases import FORCED_A
    from tests.golden_util import hip_stem_pins, reshape_masks
    B, T, H, W = 2, 16, 227, 227
    case = dict(name="api_train", B=B, T=T, H=H, W=W, seed=6, step=0, forced=FORCED_A)
    m = make_cad_model(case).cuda()
    m.train()
    x = co.synth_clips(6, 0, 0, B, T, H, W)
    coef = torch.tensor([1.0, -0.5, 0.25, 2.0])

    def user_loss(o, cf):
        det = sum((d * cf).sum() for fr in o["detections"] for d in fr)
        return (o["anomaly_scores"].sum() + 0.5 * o["direct_predictions"][:, 0].sum()
                + 0.1 * sum(o["kl_losses"]) + 1e-3 * det)

    out = m(x.cuda(), seed=77, step=3, clip0=0)
    user_loss(out, coef.cuda()).backward()
    torch.cuda.synchronize()
    eng = m.engine()
    assert eng.stem_grad_on
    masks = reshape_masks(hip_relu_masks(eng, B * T), x)
    pins = hip_stem_pins(eng, B * T, H, W)
    sd = make_cad_model(case).state_dict()
    params = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items()
              if "running" not in k and "num_batches" not in k}
    bufs = {k: v.detach().double().clone() for k, v in sd.items() if "running" in k}
    ref = co.cad_forward(params, bufs, x.double(), co.CadDraws.make(77, 3, 0, B, T), training=True,
                         relu_masks=masks, stem_pins=pins)
    assert sum(int(d.shape[0]) for fr in ref["detections"] for d in fr) > B * T  # live boxes
    user_loss(ref, coef.double()).backward()
    np.testing.assert_allclose(out["anomaly_scores"].detach().cpu().numpy(), ref["anomaly_scores"].detach().numpy(),
                               rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(out["direct_predictions"].detach().cpu().numpy(),
                               ref["direct_predictions"].detach().numpy(), rtol=1e-4, atol=1e-5)
    worst, det_live, stem_live = 0.0, False, False
    for n, p in m.named_parameters():
        pr = params[n]
        if pr.grad is None or float(pr.grad.abs().max()) == 0.0:
            assert p.grad is None or float(p.grad.abs().max()) < 1e-9, n
            continue
        assert p.grad is not None, n
        mine = p.grad.detach().cpu().double().numpy()
        if is_pre_bn_bias(n) or n == "backbone.conv1.bias":  # true gradient 0 (BN removes the mean)
            assert np.abs(mine).max() < 1e-6 * max(1.0, float(pr.grad.abs().max())) + 1e-6, n
            continue
        e = rel_l2(mine, pr.grad.numpy())
        worst = max(worst, e)
        det_live |= n.startswith("detector.")
        stem_live |= n.startswith(("backbone.conv1.", "backbone.bn1."))
        assert e <= 1e-4, f"{n}: relative L2 error {e:.3g} vs the mask-pinned oracle"
    assert det_live and stem_live
    bufs_dev = dict(m.named_buffers())
    for k in ("backbone.bn1.running_mean", "backbone.bn1.running_var"):
        np.testing.assert_allclose(bufs_dev[k].cpu().numpy(), bufs[k].numpy(), rtol=1e-5, atol=1e-6, err_msg=k)
    print(f"worst per-tensor relative L2 vs the mask-pinned oracle: {worst:.3g}")


# bf16 mode (conv_bf16 + act_bf16) is compared with the float64 oracle restating the device's bf16 rounding points
# (oracle.cad_oracle.backbone_forward_bf16: bf16 operands, bf16-stored conv outputs y, dA and dY), pinned to the
# device's ReLU decisions (the eight backbone BatchNorms and the direct classifier's four hidden layers).  What a correct
# bf16 implementation may differ from that restatement by is not a constant: a stored bf16 value flips by one ulp
# (2^-8 relative) wherever a tiny difference upstream moves it across a rounding boundary, i.e. with probability
# ~ delta / ulp, and the 16 storage points of the step (8 forward, 8 backward) cascade.  The tolerance is therefore
# derived in the test from independent implementations of the same semantics -- the restatement run in float32 (the
# device's accumulation precision), once as written and once with every conv summing its input channels in reverse
# order, both on the same pinned branch: the device must lie within BF16_SPREAD x the larger of their distances to the
# float64 restatement (+ a floor at the float32 level).  The same for the scores, the loss and the ReLU decisions (flip
# count and worst |z| at a flip, against the float32 restatements' own decisions).  Round-5 run: backbone gradients
# 0.6-1.1 x the yardstick, which itself is 0.9 % of layer1.0's weight gradient.  (History: with the
# direct classifier unpinned, one of its hidden units within 1.6e-3 rms of zero took the other branch on the device,
# which moved d_pooled and with it every backbone gradient by ~6 % and direct_classifier.3 / .6 by 5-8 % -- that
# was the earlier "bf16 drift", not the rounding cascade.)
# (BF16_SPREAD = 2.0 and the checks themselves: tests/golden_util.py, shared with test_cad_bf16_ragged_gpu.py)


def _bf16_vs_restatement(o, eng, masks, gr, x, y, sd, draws, label="config 4 per rank", det_pin=False):
    """bf16 parity of one step: the device (o, eng, gr) vs the float64 bf16 restatement, with the two float32
    restatements as the yardstick (see BF16_SPREAD; the checks are tests.golden_util.check_bf16_step).  det_pin: the
    detector MLP's hidden ReLU decisions are taken from the device too (forced-detection cases, where they carry a
    gradient).  Returns (worst gradient ratio, the references, the direct classifier's and detector's masks)."""
    # the direct classifier's ReLU decisions are the device's too (its hidden units are pinned like the backbone's: a
    # unit within rounding of zero may otherwise flip between two correct runs and move the head's weight gradients
    # by O(1) in relative terms -- round 5: one such unit moved direct_classifier.3 / .6 by 5-8 %)
    from tests.golden_util import bf16_step_references, check_bf16_step, read_debug
    B, NF = y.shape[0], x.shape[0] * x.shape[1]
    hm = [torch.from_numpy(read_debug(eng._last[0], "dir_h", i).reshape(B, w) > 0)
          for i, w in enumerate((512, 256, 128, 64))]
    dm = [torch.from_numpy(read_debug(eng._last[0], "det_h", i).reshape(NF, w) > 0)
          for i, w in enumerate((512, 256, 128, 64))] if det_pin else None
    refs = bf16_step_references(sd, x, y, draws, masks, hm, dm)
    dev = dict(final=o["final"].cpu().numpy(), probs=o["probs"].cpu().numpy(), total=float(o["losses"][4]),
               grads={n: gr[eng.slot_offset[i]:eng.slot_offset[i] + eng.slot_numel[i]].astype(np.float64)
                      for i, n in enumerate(eng.slot_names)})
    worst = check_bf16_step(dev, refs, masks, hm, draws, label, det_hm=dm)
    return worst, refs, hm, dm


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_config4_shape_per_rank(dt):
    """BASELINE config 4 per-rank workload: B=8 clips x T=32 frames x 256x256 (BN couples all 256 frames).
    fp32 mode: scores and loss within the north-star 1e-4 of the CPU oracle, every gradient tensor within relative
    L2 1e-4 of the mask-pinned float64 oracle.  bf16 mode (conv_bf16: the 3x3 convs and the frozen stem's conv1 on
    bf16 operands, fp32 accumulation; the backbone activations -- pooled stem map, conv outputs, their gradients --
    stored as bf16 (option act_bf16, on by default); BN statistics, weights, grads and the heads fp32): against the
    float64 restatement of those bf16 rounding points, within BF16_SPREAD x the distance of an independent float32
    restatement (scores, loss, every gradient tensor, ReLU decisions)."""
    B, T, H, W = 8, 32, 256, 256
    case = dict(name="cfg4", B=B, T=T, H=H, W=W, seed=9, step=1, forced=None)
    x = co.synth_clips(9, 1, 0, B, T, H, W)
    y = co.synth_labels(0, B)
    fp32 = dt == "fp32"
    m = _frozen(make_cad_model(case)).cuda().set_compute_dtype(torch.float32 if fp32 else torch.bfloat16)
    eng = m.engine()
    o = eng.forward(x.cuda(), True, 9, 1, 0, y.cuda())
    eng.backward(True)
    torch.cuda.synchronize()
    gr = eng.grads.cpu().numpy()
    from tests.golden_util import read_debug_len
    assert read_debug_len(eng._last[0], "act_bf16") == (0 if fp32 else 1)
    masks = hip_relu_masks(eng, B * T)
    draws = co.CadDraws.make(9, 1, 0, B, T)
    sd = make_cad_model(case).state_dict()
    if not fp32:
        from tests.golden_util import reshape_masks
        _bf16_vs_restatement(o, eng, reshape_masks(masks, x.double()), gr, x, y, sd, draws)
        return
    ref_grads, ref_losses, res = pinned_oracle_grads(sd, x, y, draws, masks)
    flips = check_mask_flips(masks, res["record"], x)
    print(f"config 4 per rank, fp32: ReLU decisions that differ from the float64 forward (count, worst |z|/bound) "
          f"{flips}")
    np.testing.assert_allclose(o["final"].cpu().numpy(), res["out"]["anomaly_scores"].detach().numpy(),
                               rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(o["probs"].cpu().numpy(), res["out"]["direct_predictions"].detach().numpy(),
                               rtol=1e-4, atol=1e-5)
    assert float(o["losses"][4]) == pytest.approx(float(ref_losses["total"]), rel=1e-4)
    errs = {}
    for i, n in enumerate(eng.slot_names):
        ref = ref_grads.get(n)
        mine = gr[eng.slot_offset[i]:eng.slot_offset[i] + eng.slot_numel[i]].astype(np.float64)
        if ref is None:
            assert np.abs(mine).max() == 0.0, n
            continue
        if is_pre_bn_bias(n):
            assert np.abs(mine).max() < 1e-6, n
            continue
        errs[n] = rel_l2(mine, ref.detach().numpy())
    for n, e in sorted(errs.items(), key=lambda kv: -kv[1])[:12]:
        print(f"  {dt} {n}: {e:.3g}")
    bad = {n: e for n, e in errs.items() if e > 1e-4}
    assert not bad, f"relative L2 errors above tolerance ({dt}): {bad}"
    print(f"config 4 per rank, {dt}: worst per-tensor relative L2 vs the mask-pinned oracle {max(errs.values()):.3g}")


def test_staged_backward_equals_whole_backward():
    """vad_cad_backward_stage 0 then 1 (the DP overlap path) writes the same grads, bit for bit, as one backward;
    after stage 0 every non-backbone grad is already final."""
    case = CASES[1]
    m, eng, o, grads, tn = _hip_step(case, step_opt=False)
    B, T, H, W = case["B"], case["T"], case["H"], case["W"]
    x = co.synth_clips(case["seed"], case["step"], 0, B, T, H, W).cuda()
    y = co.synth_labels(0, B).cuda()
    eng.forward(x, True, case["seed"], case["step"], 0, y)
    eng.backward(True, stage=0)
    torch.cuda.synchronize()
    nb = eng.backbone_floats
    assert 0 < nb < eng.param_floats
    assert torch.equal(eng.grads[nb:eng.param_floats + 2], grads[nb:eng.param_floats + 2])
    eng.backward(True, stage=1)
    torch.cuda.synchronize()
    assert torch.equal(eng.grads[:eng.param_floats + 2], grads[:eng.param_floats + 2])


@pytest.mark.gpu
@pytest.mark.parametrize("ci", [0, 1])
def test_stage2_backward_equals_whole_backward(ci):
    """Stage 2 (the head / detector backward left running on the plan's side stream, the backbone gated on the
    detector's input gradient only) + wait_side + stage 1 write the same grads, bit for bit, as one backward: in the
    fallback regime (no box in range: the backbone does not wait for the causal head) and the forced one (it waits
    for the detector's input gradient)."""
    case = CASES[ci]
    m, eng, o, grads, tn = _hip_step(case, step_opt=False)
    B, T, H, W = case["B"], case["T"], case["H"], case["W"]
    x = co.synth_clips(case["seed"], case["step"], 0, B, T, H, W).cuda()
    y = co.synth_labels(0, B).cuda()
    eng.forward(x, True, case["seed"], case["step"], 0, y)
    eng.backward(True, stage=2)
    side = torch.cuda.Stream()
    eng.wait_side(side)
    side.wait_stream(torch.cuda.current_stream())
    nb = eng.backbone_floats
    with torch.cuda.stream(side):
        head = eng.grads[nb:eng.param_floats + 2].clone()
    eng.backward(True, stage=1)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(head, grads[nb:eng.param_floats + 2])
    assert torch.equal(eng.grads[:eng.param_floats + 2], grads[:eng.param_floats + 2])


@pytest.mark.parametrize("ci", [0, 1])
def test_second_backward_on_one_forward(ci):
    """Two backwards with different upstream grads on one forward (autograd retain_graph=True) give the grads of two
    fresh forward + backward runs, bit for bit: the second backward re-arms the detector gate (cad_plan.hip) and
    waits for its own detector input gradient again.  Fallback and forced regimes."""
    case = CASES[ci]
    m = make_cad_model(case).cuda()
    eng = m.engine()
    B, T, H, W = case["B"], case["T"], case["H"], case["W"]
    x = co.synth_clips(case["seed"], case["step"], 0, B, T, H, W).cuda()
    g = torch.Generator().manual_seed(5)
    ups = [(torch.randn(B, generator=g).cuda(), torch.randn(B, 2, generator=g).cuda()) for _ in range(2)]
    eng.forward(x, True, case["seed"], case["step"], 0)
    shared = []
    for dc, dp in ups:
        eng.backward(False, d_causal=dc, d_probs=dp)
        shared.append(eng.grads.clone())
    fresh = []
    for dc, dp in ups:
        eng.forward(x, True, case["seed"], case["step"], 0)
        eng.backward(False, d_causal=dc, d_probs=dp)
        fresh.append(eng.grads.clone())
    torch.cuda.synchronize()
    assert not torch.equal(fresh[0], fresh[1])
    for a, b in zip(shared, fresh):
        assert torch.equal(a, b)


def test_module_api_detection_grads():
    """Detections carry autograd as in the reference (cad:201-222: each frame's boxes are slices of the rescaled
    detector output; the fallback box is a constant): a loss on out["detections"] trains the detector and the
    backbone under it.  Forced-detection weights (valid boxes), eval mode; every grad vs the mask-pinned float64
    oracle (relative L2 <= 1e-4 per tensor)."""
    from tests.golden.cases import CAD_CASES
    case = dict(next(c for c in CAD_CASES if c["name"] == "forced_b2t4_64"))
    m = make_cad_model(case).cuda()
    m.eval()
    B, T = case["B"], case["T"]
    x = co.synth_clips(case["seed"], 0, 0, B, T, case["H"], case["W"])
    coef = torch.tensor([1.0, -0.5, 0.25, 2.0])

    def user_loss(o, cf):
        return sum((d * cf).sum() for fr in o["detections"] for d in fr) + o["anomaly_scores"].sum()

    worst, live, ref = _module_pinned_check(m, case, x, user_loss, training=False, coef=coef)
    assert sum(int(d.shape[0]) for fr in ref["detections"] for d in fr) > B * T  # live boxes (forced regime)
    assert any(n.startswith("detector.") for n in live)
    print(f"worst per-tensor relative L2 vs the mask-pinned oracle: {worst:.3g}")


@pytest.mark.parametrize("H,W", [(24, 40), (16, 16)])
def test_small_frames_grads(H, W):
    """Frames so small that the final map is 1 x 2 / 1 x 1: every AdaptiveAvgPool2d((4, 6)) bin covers the same rows
    (up to 4 row bins per row in the backward), stride-2 layers on 2-wide maps.  Loss within 1e-4 and every gradient
    tensor within relative L2 1e-4 of the mask-pinned float64 oracle."""
    B, T = 2, 3
    case = dict(name="small", B=B, T=T, H=H, W=W, seed=12, step=0, forced=None)
    m = _frozen(make_cad_model(case)).cuda()
    eng = m.engine()
    x = co.synth_clips(12, 0, 0, B, T, H, W)
    y = co.synth_labels(0, B)
    o = eng.forward(x.cuda(), True, 12, 0, 0, y.cuda())
    eng.backward(True)
    torch.cuda.synchronize()
    gr = eng.grads.cpu().numpy()
    masks = hip_relu_masks(eng, B * T)
    ref_grads, ref_losses, _ = pinned_oracle_grads(make_cad_model(case).state_dict(), x, y,
                                                   co.CadDraws.make(12, 0, 0, B, T), masks)
    assert float(o["losses"][4]) == pytest.approx(float(ref_losses["total"]), rel=1e-4)
    check_pinned_grads(eng, gr, ref_grads)


@pytest.mark.parametrize("B", [1, 3, 8])
def test_dir_affine_matches_plain_backward(B):
    """Knob cad_dir_affine (the direct classifier's loss-mode backward run in the train forward as the input-gradient
    chain of the stacked rows [A; beta], folded with the causal score in the backward: cad_plan.hip, mlp.hip dir_mid /
    dir_combine) against the plain per-layer backward, B in {1, 3, 8} (rows zero-padded to 8, gate row r % B): the
    same loss, and every gradient within relative L2 per tensor of 1e-6 for the heads and 1e-5 for the backbone (only
    the fp32 summation order of the clip-mean grads differs; eight train-mode BatchNorm backwards amplify that noise:
    1.03e-6 measured on layer1.0 at B = 1)."""
    from vad_amd import _native as nat
    case = dict(name="affine", B=B, T=3, H=64, W=80, seed=21, step=2, forced=None)
    x = co.synth_clips(21, 2, 0, B, 3, 64, 80).cuda()
    y = co.synth_labels(0, B).cuda()
    runs = []
    for aff in (1, 0):
        nat.check(nat.lib().vad_set_tuning(b"cad_dir_affine", aff))
        try:
            eng = _frozen(make_cad_model(case)).cuda().engine()
            o = eng.forward(x, True, 21, 2, 0, y)
            eng.backward(True)
            torch.cuda.synchronize()
            runs.append((float(o["losses"][4]), eng.grads[:eng.param_floats].cpu().double().numpy()))
        finally:
            nat.check(nat.lib().vad_set_tuning(b"cad_dir_affine", 1))
    assert runs[0][0] == pytest.approx(runs[1][0], rel=1e-6)
    worst, live = 0.0, 0
    for i, n in enumerate(eng.slot_names):
        o, k = eng.slot_offset[i], eng.slot_numel[i]
        a, b = runs[0][1][o:o + k], runs[1][1][o:o + k]
        if not b.any():
            assert not a.any(), n
            continue
        if is_pre_bn_bias(n):  # true gradient 0: rounding noise either way
            assert np.abs(a).max() < 1e-6, n
            continue
        e = rel_l2(a, b)
        live += n.startswith("direct_classifier.")
        worst = max(worst, e)
        tol = 1e-5 if n.startswith("backbone.") else 1e-6
        assert e <= tol, f"{n}: relative L2 {e:.3g} between cad_dir_affine on and off"
    assert live >= 10  # the five layers' weights and biases carry a gradient
    print(f"B={B}: worst per-tensor relative L2 (affine vs plain) {worst:.3g}")


def test_s2_dgrad_presplit_weights_bit_identical():
    """Knob conv_dgrad_s2_w3: the stride-2 input gradients stage the weight image the prep pre-split into bf16 planes
    (hi, mid, lo of each fp32 weight, split3's arithmetic) instead of splitting it in every block: every gradient
    bit-identical."""
    from vad_amd import _native as nat
    case = dict(name="w3", B=2, T=3, H=96, W=80, seed=29, step=1, forced=None)
    x = co.synth_clips(29, 1, 0, 2, 3, 96, 80).cuda()
    y = co.synth_labels(0, 2).cuda()
    runs = []
    for on in (1, 0):
        nat.check(nat.lib().vad_set_tuning(b"conv_dgrad_s2_w3", on))
        try:
            eng = _frozen(make_cad_model(case)).cuda().engine()
            eng.forward(x, True, 29, 1, 0, y)
            eng.backward(True)
            torch.cuda.synchronize()
            runs.append(eng.grads[:eng.param_floats].cpu().clone())
        finally:
            nat.check(nat.lib().vad_set_tuning(b"conv_dgrad_s2_w3", 1))
    assert runs[0].abs().sum() > 0
    assert torch.equal(runs[0], runs[1]), float((runs[0] - runs[1]).abs().max())
