"""Float64 statement of the four fused optimizers, in stock torch.

Every train step of this project ends in a hand-written optimizer kernel (cad: AdamW over slot groups; minicausal:
Adam with coupled L2 and a gated clip; a2: AdamW that always clips; cad1: Adam that always clips, with grad_scale).
This module says what they must compute, independently of the package's engines and of the oracle's own update:
one leaf per slot, ``torch.nn.utils.clip_grad_norm_`` over the slots that have a gradient, then
``torch.optim.AdamW`` / ``torch.optim.Adam`` (``foreach=False``) on CPU.  A slot that is inactive in a step gets
``grad = None``: torch then leaves its state and its step count alone and leaves it out of the norm.

``dtype=torch.float32`` runs the same sequence in float32.  The distance of that restatement from the float64 run is
what float32 arithmetic costs on the given inputs, and it supplies the tolerance of the device tests (``bound``).

The C ABI carries every hyperparameter as a float: ``as_f32`` rounds a hyperparameter set the same way, so the
reference is asked for the betas the device is asked for (0.999 as a float is 0.99900001287..., whose ``1 - beta2``
differs from 0.001 by 1.3e-5 relative: that is a property of the inputs, not of either implementation).
"""
import math

import numpy as np
import torch

# Each model's production values (CadTrainer, StableTrainer, ImprovedMiniCausalVAD.train_step, AeTrainer).
# decoupled: AdamW (True) or Adam with the decay added to the gradient (False); clip_above: None clips on every step,
# a number clips only when the norm exceeds it (minicausal's gate).
PRODUCTION = {
    "cad": dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5, max_norm=1.0, clip_above=None,
                decoupled=True),
    "mc": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5, max_norm=1.0, clip_above=10.0,
               decoupled=False),
    "a2": dict(lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-3, max_norm=0.5, clip_above=None,
               decoupled=True),
    "ae": dict(lr=5e-7, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-6, max_norm=0.1, clip_above=None,
               decoupled=False),
}
# Every term visible above rounding: the decay against the update, eps against sqrt(v), both bias corrections.
LOUD = dict(lr=1e-2, betas=(0.8, 0.95), eps=1e-4, weight_decay=0.1)
RESUME_STEP = 20  # bias corrections still matter here (0.8**20 = 1.2e-2, 0.95**20 = 0.36, 0.999**20 = 0.98)
STEPS = 6

# Norm of the (scaled) gradient over the active slots per step; None keeps what the recipe gives; "nonfinite" puts an
# inf into one element.  One step of every schedule has norm 1e3, so the clip bites hard; minicausal's straddles
# clip_above = 10 by +-0.1 %, far outside float32's error of a norm.
NORMS = {
    "cad": [0.5, None, 1e3, 0.9, 3.0, 0.25],
    "mc": [3.0, 9.99, 10.01, 1e3, "nonfinite", 5.0],
    "a2": [0.2, 1e3, 0.49, 0.51, 2.0, 0.1],
    "ae": [0.05, 1e3, "nonfinite", 0.099, 0.2, 0.02],
}
# cad's detector / structure-learner "has a gradient" flags per step (summed over ranks, so 2.0 occurs): off, on, off,
# ... at different steps; the detector is inactive in step 1 and active in step 2, so its own step count (1) and the
# global one (2) differ
CAD_FLAGS = [(0.0, 1.0), (1.0, 0.0), (0.0, 0.0), (2.0, 1.0), (1.0, 0.0), (0.0, 1.0)]


def cad_active(groups, flags, stem=True):
    """Per step one bool per slot, from the cad engine's group codes (0 stem: active when it trains, 1 always,
    2 detector, 3 structure learner, 4 never) and the two flag floats."""
    return [[g == 1 or (g == 2 and f[0] > 0) or (g == 3 and f[1] > 0) or (g == 0 and stem) for g in groups]
            for f in flags]


def hyper(model, which):
    """The hyperparameter set `which` ("production", "loud", "resume": loud values) of `model`, as floats of the ABI."""
    h = dict(PRODUCTION[model])
    if which != "production":
        h.update(LOUD)
    return as_f32(h)


def as_f32(h):
    r = lambda v: float(np.float32(v))  # noqa: E731
    out = dict(h)
    for k in ("lr", "eps", "weight_decay", "max_norm"):
        out[k] = r(h[k])
    out["betas"] = (r(h["betas"][0]), r(h["betas"][1]))
    if h.get("clip_above") is not None:
        out["clip_above"] = r(h["clip_above"])
    return out


# ---------------------------------------------------------------------------------------------- inputs
def base_grads(seed, n, steps):
    """`steps` flat float64 gradients of n elements: magnitudes log-uniform over 1e-8 .. 1 (eps and wd * p matter
    against g), drawn once per element; every seventh element exactly zero; signs redrawn every step (exp_avg
    cancels while exp_avg_sq builds up)."""
    gen = torch.Generator().manual_seed(seed)
    mag = torch.pow(10.0, torch.rand(n, generator=gen, dtype=torch.float64) * 8.0 - 8.0)
    mag[::7] = 0.0
    return [mag * (torch.randint(0, 2, (n,), generator=gen).double() * 2.0 - 1.0) for _ in range(steps)]


def slot_norm(g, slots, active, scale=1.0):
    """Float64 norm of scale * g over the active slots."""
    tot = 0.0
    for (_, o, k), a in zip(slots, active):
        if a:
            tot += float((g[o:o + k].double() * scale).pow(2).sum())
    return math.sqrt(tot)


def make_grads(seed, n, slots, norms, active=None, grad_scale=1.0):
    """The float32 gradients of one test: base_grads rescaled per step so that grad_scale * g has the norm `norms[k]`
    over the slots active in step k; "nonfinite" steps keep their scale and get an inf in the middle of the largest
    active slot.  Elements outside every slot are zero (the backward never writes there)."""
    steps = len(norms)
    inside = torch.zeros(n, dtype=torch.bool)
    for _, o, k in slots:
        inside[o:o + k] = True
    out = []
    for step, g in enumerate(base_grads(seed, n, steps)):
        act = active[step] if active is not None else [True] * len(slots)
        g = torch.where(inside, g, torch.zeros_like(g))
        want = norms[step]
        if want is not None and want != "nonfinite":
            g = g * (want / slot_norm(g, slots, act, grad_scale))
        g = g.float()
        if want == "nonfinite":
            _, o, k = max((s for s, a in zip(slots, act) if a), key=lambda s: s[2])
            g[o + k // 2] = float("inf")
        out.append(g)
    return out


def resume_state(seed, n, slots, step=RESUME_STEP):
    """A saved optimizer state to continue from: flat exp_avg ~ 1e-3 N(0, 1), exp_avg_sq ~ 1e-5 U(0, 1) inside the
    slots (zero outside), every slot at `step`."""
    gen = torch.Generator().manual_seed(seed + 1000)
    m = torch.randn(n, generator=gen) * 1e-3
    v = torch.rand(n, generator=gen) * 1e-5
    inside = torch.zeros(n, dtype=torch.bool)
    for _, o, k in slots:
        inside[o:o + k] = True
    zero = torch.zeros(n)
    return dict(exp_avg=torch.where(inside, m, zero), exp_avg_sq=torch.where(inside, v, zero),
                steps=[step] * len(slots))


# ---------------------------------------------------------------------------------------------- the reference
def run_reference(slots, params, grads, *, lr, betas, eps, weight_decay, max_norm, clip_above=None, decoupled=True,
                  grad_scale=1.0, active=None, state=None, dtype=torch.float64):
    """slots: [(name, offset, numel)] over the flat float32 `params`; grads: one flat float32 tensor per step;
    active: per step one bool per slot (None: all); state: dict(exp_avg, exp_avg_sq flat, steps list) to continue
    from.  Returns one dict per step: params / exp_avg / exp_avg_sq (flat, `dtype`; outside the slots: the input
    params, zeros), steps (list of int), norm (pre-clip, of the scaled gradient), clipped, status (2 stepped, 1 a
    non-finite gradient: nothing changes)."""
    leaves = [params[o:o + k].detach().to(dtype).clone().requires_grad_(True) for _, o, k in slots]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls(leaves, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=False)
    if state is not None:
        for leaf, (_, o, k), st in zip(leaves, slots, state["steps"]):
            opt.state[leaf] = dict(step=torch.tensor(float(st)),
                                   exp_avg=state["exp_avg"][o:o + k].detach().to(dtype).clone(),
                                   exp_avg_sq=state["exp_avg_sq"][o:o + k].detach().to(dtype).clone())
    out = []
    for step, g in enumerate(grads):
        act = active[step] if active is not None else [True] * len(slots)
        live = []
        for leaf, (_, o, k), a in zip(leaves, slots, act):
            leaf.grad = g[o:o + k].detach().to(dtype) * grad_scale if a else None
            if a:
                live.append(leaf)
        rec = dict(norm=float("nan"), clipped=False, status=1)
        if all(bool(torch.isfinite(p.grad).all()) for p in live):
            if clip_above is None:
                rec["norm"] = float(torch.nn.utils.clip_grad_norm_(live, max_norm, foreach=False))
                rec["clipped"] = True
            else:
                # the root of the summed squares of the per-slot norms (mc:294-306), then clip_grad_norm_ behind the gate
                total = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in live]))
                rec["norm"] = float(total)
                if float(total) > clip_above:
                    torch.nn.utils.clip_grad_norm_(live, max_norm, foreach=False)
                    rec["clipped"] = True
            opt.step()
            rec["status"] = 2
        flat_p = params.detach().to(dtype).clone()
        flat_m = torch.zeros_like(flat_p)
        flat_v = torch.zeros_like(flat_p)
        counts = []
        for leaf, (_, o, k) in zip(leaves, slots):
            st = opt.state.get(leaf, {})
            flat_p[o:o + k] = leaf.detach()
            if st:
                flat_m[o:o + k] = st["exp_avg"]
                flat_v[o:o + k] = st["exp_avg_sq"]
            counts.append(int(st["step"]) if st else 0)
        rec.update(params=flat_p, exp_avg=flat_m, exp_avg_sq=flat_v, steps=counts)
        out.append(rec)
    return out


# ---------------------------------------------------------------------------------------------- the bound
BUFFERS = ("params", "exp_avg", "exp_avg_sq")


def bound(ref64, ref32, o, k, steps_done, key):
    """Limit of max|device - float64| over one slot of one buffer: twice what the float32 restatement is away from
    float64 (the margin tests/test_grad64.py gives another summation and contraction order) plus one rounding of the
    slot's largest value per step taken (so a slot of one or two elements, where the restatement can be exact, does
    not fail on an ulp)."""
    r64 = ref64[key][o:o + k]
    err32 = float((ref32[key][o:o + k].double() - r64).abs().max())
    return 2.0 * err32 + steps_done * 2.0 ** -23 * float(r64.abs().max())


def worst_ratio(got, ref64, ref32, slots, steps_done):
    """(largest distance / bound over every slot and buffer, where).  got: dict of flat tensors like a reference
    record."""
    worst, where = 0.0, None
    for name, o, k in slots:
        for key in BUFFERS:
            d = float((got[key][o:o + k].double() - ref64[key][o:o + k]).abs().max())
            b = bound(ref64, ref32, o, k, steps_done, key)
            r = d / b if b > 0.0 else (0.0 if d == 0.0 else float("inf"))
            if r > worst:
                worst, where = r, (name, key, d, b)
    return worst, where
