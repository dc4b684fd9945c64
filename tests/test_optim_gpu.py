"""The four fused optimizer kernels over several steps against stock torch in float64 (tests/optim_ref.py).

Each test builds its model at the smallest plan the engine accepts and runs one real forward and backward, so that a
plan exists, the state is bound and the weight images are fresh.  Then, for six steps, the engine's flat gradient
buffer is overwritten with a generated gradient (optim_ref.make_grads: magnitudes over eight decades, exact zeros,
signs redrawn per step, a norm schedule that clips on some steps and not on others), the engine's own
``optimizer_step`` runs, and params, exp_avg, exp_avg_sq, step counts and the norm / status outputs are copied back
and compared after every step.

The bound is measured, not chosen (optim_ref.bound): per slot and buffer,
``max|device - float64| <= 2 * max|float32 restatement - float64| + steps * 2**-23 * max|value|``.  Norms at
rel 1e-5 (as check_adamw_applied), step counts / flags / status exactly.  tests/test_optim_ref.py shows that a wrong
bias-correction step, swapped betas, a misplaced eps, a missing bias correction, the other kind of weight decay or a
slot taking the global step count all land at least ten times outside this bound on these inputs.

Hyperparameter sets: each model's production values; "loud" (lr 1e-2, betas 0.8 / 0.95, eps 1e-4, wd 0.1: every
term above rounding); "resume" (the loud values, continuing from a saved state at step 20)."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests import optim_ref as R

pytestmark = pytest.mark.gpu
SETS = ("production", "loud", "resume")


def _drive(model, which, seed, slots, n, bufs, step_fn, read_fn, kw, active=None, before_step=None):
    """bufs: the engine's flat device tensors dict(params, grads, exp_avg, exp_avg_sq, steps).  step_fn(k) runs the
    engine's optimizer step; read_fn() returns dict(norm, and clipped / status where the engine reports them).
    Returns the worst distance / bound ratio."""
    dev = {k: bufs[k] for k in R.BUFFERS}
    inside = torch.zeros(n, dtype=torch.bool)
    for _, o, k in slots:
        inside[o:o + k] = True
    state = None
    if which == "resume":
        state = R.resume_state(seed, n, slots)
        bufs["exp_avg"][:n].copy_(state["exp_avg"])
        bufs["exp_avg_sq"][:n].copy_(state["exp_avg_sq"])
        bufs["steps"].fill_(R.RESUME_STEP)
    torch.cuda.synchronize()
    prev = {k: dev[k][:n].cpu() for k in R.BUFFERS}
    prev["steps"] = bufs["steps"].cpu().tolist()
    grads = R.make_grads(seed, n, slots, R.NORMS[model], active, kw.get("grad_scale", 1.0))
    ref64 = R.run_reference(slots, prev["params"], grads, active=active, state=state, **kw)
    ref32 = R.run_reference(slots, prev["params"], grads, active=active, state=state, dtype=torch.float32, **kw)
    worst, where = 0.0, None
    for k, g in enumerate(grads):
        if before_step is not None:
            before_step(k)
        bufs["grads"][:n].copy_(g)
        step_fn(k)
        torch.cuda.synchronize()
        got = {key: dev[key][:n].cpu() for key in R.BUFFERS}
        got["steps"] = bufs["steps"].cpu().tolist()
        out = read_fn()
        want = ref64[k]
        assert got["steps"] == want["steps"], (k, got["steps"], want["steps"])
        if "status" in out:
            assert out["status"] == want["status"], k
        if want["status"] == 1:  # a non-finite gradient: counted, nothing moves
            for key in R.BUFFERS:
                assert torch.equal(got[key], prev[key]), (k, key)
            prev = got
            continue
        assert out["norm"] == pytest.approx(want["norm"], rel=1e-5), k
        if "clipped" in out:
            assert out["clipped"] == want["clipped"], (k, out["norm"])
        act = active[k] if active is not None else [True] * len(slots)
        for key in R.BUFFERS:
            assert torch.equal(got[key][~inside], prev[key][~inside]), (k, key, "padding between the slots moved")
            for (name, o, m), a in zip(slots, act):
                if not a:
                    assert torch.equal(got[key][o:o + m], prev[key][o:o + m]), (k, key, name, "inactive slot moved")
        ratio, w = R.worst_ratio(got, want, ref32[k], slots, k + 1)
        if ratio > worst:
            worst, where = ratio, (k,) + w
        prev = got
    print(f"optimizer {model}/{which}: worst distance / bound = {worst:.3f} at (step, slot, buffer, distance, bound) "
          f"{where}")
    assert worst <= 1.0, where
    return worst


# ---------------------------------------------------------------------------------------------- cad
def _cad_model(frozen):
    from vad_amd.cad import CausalAnomalyDetector
    from vad_amd.train import apply_memory_efficient_training
    torch.manual_seed(0)
    m = CausalAnomalyDetector()
    if frozen:
        with contextlib.redirect_stdout(io.StringIO()):
            apply_memory_efficient_training(m)
    return m


# (hyperparameters, stem frozen, grad_scale, opt_images): both stems, both scales and both image modes occur
@pytest.mark.parametrize("which,frozen,grad_scale,opt_images",
                         [("production", True, 1.0, 1), ("loud", False, 0.5, 0), ("resume", False, 1.0, 1),
                          ("loud", True, 0.5, 1)],
                         ids=["production-frozen-images", "loud-stem-scale-noimages", "resume-stem-images",
                              "loud-frozen-scale-images"])
def test_cad_adamw_matches_float64(which, frozen, grad_scale, opt_images):
    """AdamW over slot groups: the detector and structure-learner groups go off and on at different steps, their
    gradient ranges hold non-zero values while they are off; per-slot step counts, bit-unchanged inactive slots and
    padding, total_norm over the active slots only.  After the last step one more forward must equal, bit for bit,
    that of a fresh engine loaded with the stepped parameters: the weight images the steps wrote (opt_images 1) or
    left to the relayout (0) hold exactly the parameters."""
    from oracle import cad_oracle as co
    from vad_amd import _native as nat
    B, T, H, W = 2, 2, 16, 16
    m = _cad_model(frozen).cuda()
    eng = m.engine()
    eng.init_optimizer_state()  # (before the first forward, as CadTrainer does: binding clears the fresh images)
    x = co.synth_clips(0, 0, 0, B, T, H, W).cuda()
    y = co.synth_labels(0, B).cuda()
    eng.forward(x, True, 0, 0, 0, y)
    eng.backward(True)
    nat.check(nat.lib().vad_cad_set_option(eng._last[0].h, b"opt_images", opt_images))
    assert eng.stem_grad_on == (not frozen)
    n = eng.param_floats
    slots = list(zip(eng.slot_names, eng.slot_offset, eng.slot_numel))
    active = R.cad_active(eng.slot_group, R.CAD_FLAGS, stem=not frozen)
    assert any(g == 0 for g in eng.slot_group) and any(g == 2 for g in eng.slot_group)
    assert any(g == 3 for g in eng.slot_group)
    kw = R.hyper("cad", which)
    kw["grad_scale"] = grad_scale
    tn = torch.zeros(1, device="cuda")
    bufs = dict(params=eng.params, grads=eng.grads, exp_avg=eng.exp_avg, exp_avg_sq=eng.exp_avg_sq, steps=eng.steps)

    def step(k):
        eng.grads[n:n + 2].copy_(torch.tensor(R.CAD_FLAGS[k]))
        eng.optimizer_step(kw["lr"], kw["betas"], kw["eps"], kw["weight_decay"], kw["max_norm"], grad_scale,
                           total_norm=tn)

    _drive("cad", which, 11, slots, n, bufs, step, lambda: dict(norm=float(tn)), kw, active)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    o1 = eng.forward(x, True, 5, 1, 0, y)
    fresh = _cad_model(frozen)
    fresh.load_state_dict(sd)
    o2 = fresh.cuda().engine().forward(x, True, 5, 1, 0, y)
    torch.cuda.synchronize()
    for key in ("final", "probs", "causal", "kl", "z", "adj", "boxes", "losses"):
        assert torch.equal(o1[key], o2[key]), key


# ---------------------------------------------------------------------------------------------- minicausal
@pytest.mark.parametrize("which", SETS)
def test_mc_adam_matches_float64(which):
    """Adam with coupled L2 behind the gated clip: norms just below and just above clip_above (flag and coefficient
    follow), a step with an inf in one gradient element (status 1, nothing moves, the next finite step continues from
    the untouched count).  A real forward precedes every step: it arms the status and clipped words, which live in
    the plan's workspace."""
    from oracle import mc_oracle as mo
    from tests.test_mc_oracle import make_mc_model
    case = dict(B=2, T=8, H=16, W=16, seed=3, step=0, scale=1.0)
    model = make_mc_model(case).cuda().train()
    x = mo.synth_clips(3, 0, 0, 2, 8, 16, 16).cuda().contiguous()
    y = mo.synth_labels(0, 2).cuda().float().contiguous()
    e = model.engine(x)
    e.forward(x, True, 3, 0, 0, labels=y)
    e.backward()
    n = e.params.numel()
    kw = R.hyper("mc", which)
    bufs = dict(params=e.params, grads=e.grads, exp_avg=e.exp_avg, exp_avg_sq=e.exp_avg_sq, steps=e.steps)

    def step(k):
        e.optimizer_step(kw["lr"], wd=kw["weight_decay"], b1=kw["betas"][0], b2=kw["betas"][1], eps=kw["eps"],
                         clip_above=kw["clip_above"], max_norm=kw["max_norm"])

    def read():
        l = e.losses.cpu().tolist()
        return dict(norm=l[1], clipped=bool(l[2]), status=int(l[3]))

    _drive("mc", which, 12, e.slots, n, bufs, step, read, kw,
           before_step=lambda k: e.forward(x, True, 3, k + 1, 0, labels=y))


# ---------------------------------------------------------------------------------------------- a2
@pytest.mark.parametrize("which", SETS)
def test_a2_adamw_matches_float64(which):
    """AdamW (decoupled decay) that clips at max_norm on every step; losses[8] carries the norm."""
    from oracle import a2_oracle as ao
    from tests.test_a2_oracle import make_a2_model
    case = dict(B=2, T=8, H=16, W=16, seed=25, step=0, ckpt=False)
    model = make_a2_model(case).to("cuda").train()
    x = ao.synth_clips(25, 0, 0, 2, 8, 16, 16).cuda().float().contiguous()
    e = model.engine(x)
    e.forward(x, True, 25, 0, 0, with_loss=True)
    e.backward()
    torch.cuda.synchronize()
    assert np.isfinite(float(e.losses[0]))  # (status 2: the optimizer steps)
    n = e.params.numel()
    kw = R.hyper("a2", which)
    bufs = dict(params=e.params, grads=e.grads, exp_avg=e.exp_avg, exp_avg_sq=e.exp_avg_sq, steps=e.steps)

    def step(k):
        e.optimizer_step(kw["lr"], kw["weight_decay"], kw["max_norm"], kw["betas"], kw["eps"])

    _drive("a2", which, 13, e.slots, n, bufs, step, lambda: dict(norm=float(e.losses[8])), kw)


# ---------------------------------------------------------------------------------------------- cad1 autoencoder
@pytest.mark.parametrize("which", SETS)
def test_ae_adam_matches_float64(which):
    """Adam (coupled decay) that always clips, with grad_scale 0.5 and max_norm 0.1: the reported norm is that of the
    scaled gradient; a non-finite gradient step has status 1 and changes nothing."""
    from oracle import ae_oracle as ae
    from tests.test_ae_oracle import make_ae_model
    case = dict(B=1, T=2, seed=47, lr=5e-7, labels=[[0]], val_labels=[0], test_labels=[0], mem=(20, 20))
    model = make_ae_model(case).cuda().train()
    e = model.engine()
    e.init_optimizer_state()
    x = ae.synth_clips(47, 0, 0, 1, 2).cuda()
    e.forward(x, stages=3, training=True, loss_mode=2, outputs=False)
    e.backward(True)
    n = e.params.numel()
    kw = R.hyper("ae", which)
    kw["grad_scale"] = 0.5
    bufs = dict(params=e.params, grads=e.grads, exp_avg=e.exp_avg, exp_avg_sq=e.exp_avg_sq, steps=e.steps)

    def step(k):
        e.optimizer_step(kw["lr"], kw["weight_decay"], kw["max_norm"], kw["betas"], kw["eps"], grad_scale=0.5)

    def read():
        l = e.losses.cpu().tolist()
        return dict(norm=l[1], clipped=bool(l[2]), status=int(l[3]))

    _drive("ae", which, 14, e.slots, n, bufs, step, read, kw,
           before_step=lambda k: e.forward(x, stages=3, training=True, loss_mode=2, outputs=False))
