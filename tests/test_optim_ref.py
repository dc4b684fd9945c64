"""Host-only: the inputs of tests/test_optim_gpu.py can see the optimizer bugs they are there for.

A hand-written float64 Adam / AdamW (`run_manual`) first has to reproduce tests/optim_ref.py's stock-torch reference;
then each of seven deliberate changes to it must land at least ten times outside the bound the GPU tests allow
(optim_ref.bound: twice the float32 restatement's own distance plus one rounding per step), in at least one of the
parametrised cases (four optimizers x production / loud / resume hyperparameters), on the same gradient recipe, norm
schedule and flag schedule the GPU tests use."""
import functools
import math

import pytest
import torch

from tests import optim_ref as R

N = 4096
# (name, offset, numel, group) with the cad engine's group codes: 1 always, 2 detector, 3 structure learner.  Slots of
# one and two elements, 256-aligned offsets with padding between them, as in the engines' flat buffers.
SLOTS4 = [("w0", 0, 1500, 1), ("b0", 1536, 2, 1), ("det", 1792, 1200, 2), ("s", 3072, 1, 3), ("w1", 3328, 700, 1)]
SLOTS = [s[:3] for s in SLOTS4]
MODELS = ("cad", "mc", "a2", "ae")
SETS = ("production", "loud", "resume")
MUTANTS = ("bc_step_off_by_one", "betas_swapped", "eps_inside_root", "eps_before_bc2", "no_bc2", "decay_swapped",
           "inactive_takes_global_step")


def run_manual(slots, params, grads, *, lr, betas, eps, weight_decay, max_norm, clip_above=None, decoupled=True,
               grad_scale=1.0, active=None, state=None, mutant=None):
    """Adam / AdamW written out in float64, with one optional deliberate change.  Same records as run_reference."""
    b1, b2 = betas
    if mutant == "betas_swapped":
        b1, b2 = b2, b1
    if mutant == "decay_swapped":
        decoupled = not decoupled
    p = [params[o:o + k].double().clone() for _, o, k in slots]
    if state is None:
        m = [torch.zeros_like(x) for x in p]
        v = [torch.zeros_like(x) for x in p]
        t = [0] * len(slots)
    else:
        m = [state["exp_avg"][o:o + k].double().clone() for _, o, k in slots]
        v = [state["exp_avg_sq"][o:o + k].double().clone() for _, o, k in slots]
        t = list(state["steps"])
    global_step = max(t)
    out = []
    for step, g in enumerate(grads):
        act = active[step] if active is not None else [True] * len(slots)
        gs = [g[o:o + k].double() * grad_scale if a else None for (_, o, k), a in zip(slots, act)]
        rec = dict(norm=float("nan"), clipped=False, status=1)
        if all(bool(torch.isfinite(x).all()) for x in gs if x is not None):
            norm = math.sqrt(sum(float(x.pow(2).sum()) for x in gs if x is not None))
            rec["norm"] = norm
            coef = 1.0
            if clip_above is None or norm > clip_above:
                coef = min(1.0, max_norm / (norm + 1e-6))
                rec["clipped"] = True
            global_step += 1
            for i, x in enumerate(gs):
                if x is None:
                    continue
                x = x * coef
                if decoupled:
                    p[i] = p[i] * (1.0 - lr * weight_decay)
                else:
                    x = x + weight_decay * p[i]
                m[i] = m[i] + (1.0 - b1) * (x - m[i])
                v[i] = b2 * v[i] + (1.0 - b2) * x * x
                t[i] += 1
                tb = t[i]
                if mutant == "bc_step_off_by_one":
                    tb = t[i] + 1
                if mutant == "inactive_takes_global_step":
                    tb = global_step
                bc1, bc2 = 1.0 - b1 ** tb, 1.0 - b2 ** tb
                if mutant == "eps_inside_root":
                    denom = torch.sqrt(v[i] / bc2 + eps)
                elif mutant == "eps_before_bc2":
                    denom = (torch.sqrt(v[i]) + eps) / math.sqrt(bc2)
                elif mutant == "no_bc2":
                    denom = torch.sqrt(v[i]) + eps
                else:
                    denom = torch.sqrt(v[i]) / math.sqrt(bc2) + eps
                p[i] = p[i] - (lr / bc1) * m[i] / denom
            rec["status"] = 2
        flat = {k: (params.double().clone() if k == "params" else torch.zeros(params.numel(), dtype=torch.float64))
                for k in R.BUFFERS}
        for i, (_, o, k) in enumerate(slots):
            flat["params"][o:o + k] = p[i]
            flat["exp_avg"][o:o + k] = m[i]
            flat["exp_avg_sq"][o:o + k] = v[i]
        rec.update(flat, steps=list(t))
        out.append(rec)
    return out


@functools.lru_cache(maxsize=None)
def case(model, which):
    """(kwargs of the runs, grads, float64 records, float32 records) of one parametrised case."""
    seed = 100 * MODELS.index(model) + SETS.index(which)
    gen = torch.Generator().manual_seed(seed)
    params = torch.zeros(N)
    for _, o, k in SLOTS:
        params[o:o + k] = torch.randn(k, generator=gen) * 0.1
    kw = R.hyper(model, which)
    kw["grad_scale"] = 0.5 if model == "ae" or (model == "cad" and which == "loud") else 1.0
    kw["active"] = R.cad_active([s[3] for s in SLOTS4], R.CAD_FLAGS) if model == "cad" else None
    kw["state"] = R.resume_state(seed, N, SLOTS) if which == "resume" else None
    grads = R.make_grads(seed, N, SLOTS, R.NORMS[model], kw["active"], kw["grad_scale"])
    ref64 = R.run_reference(SLOTS, params, grads, **kw)
    ref32 = R.run_reference(SLOTS, params, grads, dtype=torch.float32, **kw)
    return params, kw, grads, ref64, ref32


def ratio_of(model, which, mutant):
    params, kw, grads, ref64, ref32 = case(model, which)
    recs = run_manual(SLOTS, params, grads, mutant=mutant, **kw)
    return max(R.worst_ratio(rec, ref64[k], ref32[k], SLOTS, k + 1)[0] for k, rec in enumerate(recs)), recs


@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("model", MODELS)
def test_reference_is_adam_as_written(model, which):
    """The stock-torch reference and Adam written out by hand agree to float64 rounding, in every record field; the
    schedules do what they are there for (a clipped and an unclipped step, the gate on both sides, a skipped step
    that the next one continues from, a slot whose count falls behind the global one)."""
    params, kw, grads, ref64, ref32 = case(model, which)
    ratio, recs = ratio_of(model, which, None)
    assert ratio < 1e-3, ratio
    base = R.RESUME_STEP if which == "resume" else 0
    for k, (a, b) in enumerate(zip(recs, ref64)):
        assert a["steps"] == b["steps"] and a["status"] == b["status"] and a["clipped"] == b["clipped"], k
        assert b["steps"] == ref32[k]["steps"] and b["status"] == ref32[k]["status"], k
        assert b["clipped"] == ref32[k]["clipped"], k
        want = R.NORMS[model][k]
        if want == "nonfinite":
            assert b["status"] == 1 and b["steps"] == ref64[k - 1]["steps"], k
            for key in R.BUFFERS:
                assert torch.equal(b[key], ref64[k - 1][key]), (k, key)
            continue
        assert a["norm"] == pytest.approx(b["norm"], rel=1e-12), k
        assert ref32[k]["norm"] == pytest.approx(b["norm"], rel=1e-5), k
        if want is not None:
            assert b["norm"] == pytest.approx(want, rel=1e-6), k
    skipped = sum(1 for w in R.NORMS[model] if w == "nonfinite")
    assert ref64[-1]["steps"][0] == base + R.STEPS - skipped
    if model == "cad":
        det = [s[0] for s in SLOTS].index("det")
        assert [r["steps"][det] - base for r in ref64] == [0, 1, 1, 2, 3, 3]
    if model == "mc":
        assert [r["clipped"] for r in ref64] == [False, False, True, True, False, False]


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutant_lands_outside_the_bound(mutant):
    """Each deliberate change is at least 10x outside the GPU tests' bound in at least one case."""
    ratios = {}
    for model in MODELS:
        for which in SETS:
            if mutant == "inactive_takes_global_step" and model != "cad":
                continue  # every slot of the other three steps on every step
            ratios[(model, which)] = ratio_of(model, which, mutant)[0]
    print(mutant, {f"{m}/{w}": f"{r:.3g}" for (m, w), r in ratios.items()})
    assert max(ratios.values()) >= 10.0, ratios


@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("model", MODELS)
def test_float32_restatement_meets_the_bound_with_room(model, which):
    """By construction the float32 restatement sits at no more than half the bound; what is checked here is that the
    bound stays tight: nowhere more than 1e-5 of the buffer's largest value (the parity level of the forward and
    backward paths is 1e-4), so it cannot hide an error of the size the mutants make."""
    params, kw, grads, ref64, ref32 = case(model, which)
    for k in range(R.STEPS):
        ratio, where = R.worst_ratio(ref32[k], ref64[k], ref32[k], SLOTS, k + 1)
        assert ratio <= 0.5, (k, where)
        for key in R.BUFFERS:
            top = float(ref64[k][key].abs().max())
            for name, o, n in SLOTS:
                assert R.bound(ref64[k], ref32[k], o, n, k + 1, key) <= 1e-5 * top, (k, name, key)
