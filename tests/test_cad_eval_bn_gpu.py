"""The cad eval path (clip forward and backward, score_video, live stream, stream group) under a trained-like BatchNorm
state, against the float64 oracle.

Every other cad eval test builds its model with make_cad_model alone, so all nine BatchNorm layers are in their
constructor state (mean 0, variance 1, gamma 1, beta 0) and eval BatchNorm is y / sqrt(1 + 1e-5): a running mean that
is ignored or read from a neighbouring layer, an eps that is dropped, a shift that is lost, the frozen stem's min arm,
the eval branch of the BatchNorm backward and state kept from before a load_state_dict are all invisible there.  Here
the state is tests.golden_util.calibrated_bn_state: running statistics of the layers' own pre-BN maps (variance ~1e4
at bn1, 0.07-0.25 above it; median |mean| / std 0.9 at bn1, 1.3 at layer1.1, 0.35-0.47 above), perturbed; gamma of
either sign; beta ~ N(0, 0.3); two channels per layer whose invstd is decided by eps.

The bound on outputs and gradients is the ragged files' form, never a fixed number: F32_SPREAD (4.0) x the larger
distance of two float32 restatements of the oracle (channel sums as written / reversed) from the float64 oracle, plus
a 1e-6 floor; gradients are held to the suite's relative L2 1e-4 per tensor as well.  The folded statistics (mean,
invstd, scale, shift) are formed in double by bn_finalize_kernel and rounded once: 1 float32 ulp of the float64 value.

How the bound relates to the suite's forward tolerance rtol 1e-4 / atol 1e-5 (CPU, the float32 restatements alone,
printed by test_references_stay_inside_the_bounds as "old tolerance used"): see FINDINGS below.

FINDINGS (CPU, float32 restatements against the float64 oracle under the calibrated state)
  * Outputs: the old tolerance holds with room to spare.  Over the five clip cases and the two video cases the float32
    restatements lie 1e-8 .. 1.8e-7 from the float64 oracle on scores, probabilities, KL terms, adjacency and factors
    (boxes, coordinates of order 100: 2.7e-5) and use at most 0.27 % of rtol 1e-4 / atol 1e-5.  The bound applied here,
    4 x that distance + 1e-6, comes to 1.0-1.4e-6 absolute: about ten times tighter than the old atol.  First device
    run (MI355X): every output within 0.07-0.46 of the bound.
  * Gradients: every tensor of the restatements and of the device is far inside relative L2 1e-4 (device worst 1.2e-5).
    Under the spread bound a BatchNorm weight gradient is taken as gamma * d gamma (check_eval_clip has the reason):
    on the plain tensor the two eps-regime channels, xhat = (y - mean) / sqrt(1e-7 + eps), are 1e2-3e4 times the
    others and decide its L2, and the two float32 restatements then differ by up to 6 x from each other (forced_64
    bn1.weight 1.76e-6 / 2.95e-7, layer3.4.weight 8.86e-6 / 2.96e-6), so that neither they nor the device (bn1.weight
    1.16e-5, layer1.1.weight 3.46e-6) stay inside any spread; weighted, the restatements agree within 1.2 x on every
    BatchNorm weight and each plays the device against the other at spread 2.0 with a worst ratio to the bound of
    0.58.  Device run (MI355X): worst ratio to the bound 0.37-0.86 over the five clip cases.
  * Folded statistics: bn_finalize_kernel used to take eps as a float (1e-5f = 9.99999975e-6) where nn.BatchNorm2d and
    the float64 formula have 1e-5.  At 64x64 that left the device within 0.90 ulp; at 24x40 layer3.1's shift, a
    difference of large terms, was 4.57 ulp of its own value off (the same figures come out of the formula evaluated
    with the float eps on the CPU).  The kernel now takes eps as a double and the cad plan passes 1e-5: 0.5 ulp in
    every case.

Which assertion catches which fault (test_injected_faults_are_caught; float32 restatement with one EVAL_BN_FAULTS entry
at BatchNorm 0 = bn1, 2 = layer1.4 behind a stride-1 conv, 3 = layer2.1 behind a stride-2 conv; case forced_64, the
frozen-stem fault on forced_64_frozen):
  fault                 BatchNorm 0                      BatchNorm 2                      BatchNorm 3
  mean_ignored          counts, folded statistics        counts, folded statistics        counts, folded statistics
  neighbour_buffers     counts, folded statistics        counts, folded statistics        counts, folded statistics
  eps_dropped           counts, folded statistics        counts, folded statistics        counts, folded statistics
  beta_dropped          counts, folded statistics        counts, folded statistics        counts, folded statistics
  stale_state           counts, folded statistics        counts, folded statistics        counts, folded statistics
  gamma_sign_in_stem    counts (frozen case)             -                                -
  train_backward        gradient bound, relative L2      gradient bound, relative L2      gradient bound, relative L2
  bias_grad_zero        gradient bound, relative L2      gradient bound, relative L2      gradient bound, relative L2
  (counts: the faulted forward changes a frame's box count, after which no output is compared.)

Worst device / bound ratios of the GPU run are in the docstrings of the GPU tests.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import cad_oracle as co
from tests.golden.cases import FORCED_A
from tests.golden_util import (F32_SPREAD, calibrated_bn_state, first_max_pool_idx, make_cad_model, rel_l2)
from tests.test_score_video_gpu import THRESHOLDS, TOL, _check_against_oracle

FLOOR = 1e-6          # the floor of the bound on outputs (absolute) and gradients (relative L2), as the ragged files'
COEF = torch.tensor([1.0, -0.5, 0.25, 2.0])
FAULT_BNS = (0, 2, 3)  # bn1, a BatchNorm behind a stride-1 conv, one behind a stride-2 conv
BN_WEIGHTS = {bn + ".weight" for bn in co.BN_LAYERS}
OUT_KEYS = ("anomaly_scores", "direct_predictions", "causal_anomaly_scores", "kl_losses", "adjacency_matrices",
            "causal_factors", "detections")

CLIP_CASES = [
    dict(name="fallback_64", B=2, T=4, H=64, W=64, seed=0, forced=None, frozen=False),
    dict(name="forced_64", B=2, T=4, H=64, W=64, seed=1, forced=FORCED_A, frozen=False),
    dict(name="fallback_24x40", B=2, T=3, H=24, W=40, seed=12, forced=None, frozen=False),
    dict(name="forced_24x40", B=2, T=3, H=24, W=40, seed=12, forced=FORCED_A, frozen=False),
    # the trainer's frozen stem: the fused stem kernel (max / min arm by gamma's sign), no stem gradients
    dict(name="forced_64_frozen", B=2, T=4, H=64, W=64, seed=1, forced=FORCED_A, frozen=True),
]
CLIP_IDS = [c["name"] for c in CLIP_CASES]

# Model, frame and BatchNorm-state seed of the forced video case.  Scanned with the oracle alone on the CPU (calibrated
# state, 96x80, N = 13, T = 5, stride 2; seed = model seed = frame seed = state seed) from 100 upwards: 100-104 give every
# window the same Nmax (4 or 5); 105 is the first seed that meets all the fixture conditions: Nmax [3, 3, 4, 4, 3], 77
# boxes on the 25 window frames, margin 8.6e-3 px, every layer's post-BN rms 1.06-1.51 and ReLU-on fraction 0.49-0.53.
VIDEO_FORCED_SEED = 105
VIDEO_CASES = {
    "fallback": dict(name="sv_fallback", seed=0, forced=None, H=64, W=64, N=11, T=4, stride=1, chunk=4, frozen=False,
                     key=(7, 0, 3)),
    "forced": dict(name="sv_forced", seed=VIDEO_FORCED_SEED, forced=FORCED_A, H=96, W=80, N=13, T=5, stride=2, chunk=6,
                   frozen=True, key=(11, 2, 5)),
}


def user_loss(o, cf):
    """Scores, probabilities, KL terms and the detections: every parameter with a gradient in the regime gets one."""
    det = sum((d * cf).sum() for fr in o["detections"] for d in fr)
    return (o["anomaly_scores"].sum() + 0.5 * o["direct_predictions"][:, 0].sum() + 0.1 * sum(o["kl_losses"])
            + 1e-3 * det)


# ---------------------------------------------------------------------------------------------- references
def _split(sd, dtype, grad=False):
    p = {k: v.detach().to(dtype).clone().requires_grad_(grad) for k, v in sd.items()
         if "running" not in k and "num_batches" not in k}
    bufs = {k: v.detach().to(dtype).clone() for k, v in sd.items() if "running" in k}
    return p, bufs


@functools.lru_cache(maxsize=None)
def _clip_inputs(name):
    case = next(c for c in CLIP_CASES if c["name"] == name)
    x = co.synth_clips(case["seed"], 0, 0, case["B"], case["T"], case["H"], case["W"])
    sd = calibrated_bn_state(make_cad_model(case).state_dict(), case, case["seed"])
    return case, x, co.CadDraws.make(0, 0, 0, case["B"], case["T"]), sd


def eval_run(sd, x, draws, masks, pins, dtype=torch.float64, reverse=False, eval_fault=None):
    """One eval forward and the backward of user_loss through the oracle, pinned to the given ReLU decisions (and the
    training stem's, pins).  Returns dict(out, grads {name: tensor or None}, rec)."""
    p, bufs = _split(sd, dtype, grad=True)
    rec = {}
    out = co.cad_forward(p, bufs, x.to(dtype), draws, training=False, relu_masks=masks, stem_pins=pins,
                         reverse_channels=reverse, eval_fault=eval_fault, record=rec)
    user_loss(out, COEF.to(dtype)).backward()
    return dict(out=out, grads={n: t.grad for n, t in p.items()}, rec=rec)


def clip_references(sd, x, draws, masks, pins):
    """The float64 oracle and its two float32 restatements on one pinned branch."""
    return dict(ref=eval_run(sd, x, draws, masks, pins),
                a1=eval_run(sd, x, draws, masks, pins, dtype=torch.float32),
                a2=eval_run(sd, x, draws, masks, pins, dtype=torch.float32, reverse=True))


def own_decisions(sd, x, draws, frozen):
    """The float64 eval forward's own ReLU decisions: (the eight masks, the training stem's pins or None)."""
    p, bufs = _split(sd, torch.float64)
    rec = {}
    with torch.no_grad():
        co.cad_forward(p, bufs, x.double(), draws, training=False, record=rec)
    masks = [rec[f"z{l}"] > 0 for l in range(8)]
    if frozen:
        return masks, None, rec
    z = rec["z_stem"]
    idx = first_max_pool_idx(np.ascontiguousarray(torch.relu(z).permute(0, 2, 3, 1).numpy()))
    return masks, (z > 0, torch.from_numpy(idx).permute(0, 3, 1, 2).contiguous()), rec


@functools.lru_cache(maxsize=None)
def _cpu_clip_references(name):
    case, x, draws, sd = _clip_inputs(name)
    masks, pins, rec = own_decisions(sd, x, draws, case["frozen"])
    return masks, pins, rec, clip_references(sd, x, draws, masks, pins)


def flat_outputs(o):
    """{key of OUT_KEYS: (float64 vector, the shapes it was joined from)} of a module or oracle output dict."""
    def vec(ts):
        ts = [t.detach().cpu().double().reshape(-1).numpy() for t in ts]
        return np.concatenate(ts) if ts else np.zeros(0)
    groups = {"anomaly_scores": [o["anomaly_scores"]], "direct_predictions": [o["direct_predictions"]],
              "causal_anomaly_scores": [o["causal_anomaly_scores"]], "kl_losses": list(o["kl_losses"]),
              "adjacency_matrices": list(o["adjacency_matrices"]), "causal_factors": list(o["causal_factors"]),
              "detections": [d for fr in o["detections"] for d in fr]}
    return {k: (vec(ts), [tuple(t.shape) for t in ts]) for k, ts in groups.items()}


def restatement_as_device(run, frozen=False):
    """An oracle run in the form check_eval_clip takes for the device (a missing gradient reads as zeros; frozen: the
    stem's parameters take none)."""
    return dict(out=flat_outputs(run["out"]),
                grads={n: (np.zeros(0) if g is None else g.detach().double().numpy().reshape(-1))
                       for n, g in run["grads"].items() if not (frozen and n.startswith(co.FROZEN_PREFIXES))},
                fold=[tuple(t.numpy() for t in run["rec"][f"fold{i}"]) for i in range(9)])


def old_tolerance_used(v, r):
    """max |v - r| / (1e-5 + 1e-4 |r|): at most 1 where the suite's forward tolerance holds."""
    return float((np.abs(v - r) / (TOL["atol"] + TOL["rtol"] * np.abs(r))).max()) if r.size else 0.0


# ---------------------------------------------------------------------------------------------- the assertions
def check_fold(fold, sd, label):
    """The folded state of all nine layers (per layer (mean, invstd, scale, shift), float32) against the float64
    formula on the loaded state: 1 float32 ulp of the float64 value per entry, the eps-regime channels included.
    Returns (worst distance in ulp, failures)."""
    worst, bad = 0.0, []
    for i, bn in enumerate(co.BN_LAYERS):
        rm, rv, g, b = (sd[bn + s].detach().double().numpy() for s in (".running_mean", ".running_var", ".weight",
                                                                        ".bias"))
        inv = 1.0 / np.sqrt(rv + 1e-5)
        scale = g * inv
        want = (rm, inv, scale, b - rm * scale)
        assert int((rv == np.float32(1e-7)).sum()) == 2, f"fixture, not kernel: {bn} has no two eps-regime channels"
        for name, got, w in zip(("mean", "invstd", "scale", "shift"), fold[i], want):
            ulp = np.spacing(np.abs(w).astype(np.float32)).astype(np.float64)
            d = float((np.abs(got.astype(np.float64) - w) / ulp).max())
            worst = max(worst, d)
            if not d <= 1.0:
                bad.append(("folded statistics", f"{label}: {bn} {name}: {d:.3g} ulp from the float64 formula"))
    return worst, bad


def check_eval_clip(dev, refs, yards, spread, label, frozen, sd, quiet=False):
    """One eval clip forward + backward: dev (restatement_as_device's form) against refs["ref"], the float32
    restatements named by yards as the yardstick.  Box counts and Nmax equal; every output within spread x the
    yardsticks' largest distance + FLOOR (max abs); every gradient tensor within spread x the yardsticks' largest
    relative L2 distance + FLOOR, and within relative L2 1e-4.  Under the spread bound a BatchNorm weight gradient is
    taken as gamma * d gamma, the gradient with respect to log |gamma| (sd: the loaded state, whose gamma is exact on
    both sides): d gamma_c = sum dZ xhat scales with 1 / gamma_c at a fixed output scale, so in an eps-regime channel,
    gamma ~ 1e-2 .. 1e-4 of the others', it is 1e2 .. 1e4 times the others' and the plain L2 of the tensor is decided
    by those two elements alone -- two correct float32 runs then differ by up to 6 x in it (1.76e-6 / 2.95e-7 on
    forced_64's bn1.weight) and no spread bound holds, while the other C - 2 channels go unjudged.  Weighted by gamma
    every channel counts by its effect on the layer's output, and the two float32 runs agree within 1.2 x on every
    BatchNorm weight of every case.  The relative L2 1e-4 is taken on the plain tensor, as elsewhere in the suite.
    Returns (worst device / bound ratio, failures as (assertion, text))."""
    r64 = flat_outputs(refs["ref"]["out"])
    ys = [flat_outputs(refs[k]["out"]) for k in yards]
    worst, bad = 0.0, []
    for k in OUT_KEYS:
        if dev["out"][k][1] != r64[k][1]:
            bad.append(("counts", f"{label}: {k} shapes {dev['out'][k][1]} vs the oracle's {r64[k][1]}"))
    if bad:
        return float("inf"), bad
    for k in OUT_KEYS:
        r = r64[k][0]
        if r.size == 0:
            continue
        d = float(np.abs(dev["out"][k][0] - r).max())
        yard = max(float(np.abs(y[k][0] - r).max()) for y in ys)
        bound = spread * yard + FLOOR
        worst = max(worst, d / bound)
        if not quiet:
            print(f"  {label} {k}: device {d:.3g}, float32 restatements {yard:.3g}, bound {bound:.3g}; old tolerance "
                  f"used: device {old_tolerance_used(dev['out'][k][0], r):.3g}, restatements "
                  f"{max(old_tolerance_used(y[k][0], r) for y in ys):.3g}")
        if not d <= bound:
            bad.append((f"output {k}", f"{label}: {k}: {d:.3g} > {spread} x {yard:.3g} + {FLOOR:g}"))
    for n, r in refs["ref"]["grads"].items():
        mine = dev["grads"].get(n)
        if frozen and n.startswith(co.FROZEN_PREFIXES):
            if not (mine is None or mine.size == 0):
                bad.append(("frozen", f"{label}: {n} is frozen and has a gradient"))
            continue
        if r is None or float(r.abs().max()) == 0.0:
            if not (mine is None or mine.size == 0 or float(np.abs(mine).max()) < 1e-9):
                bad.append(("gradient liveness", f"{label}: {n} has a gradient where the oracle has none"))
            continue
        r = r.detach().numpy().reshape(-1)
        if mine is None or mine.size == 0:
            mine = np.zeros_like(r)
        plain = rel_l2(mine, r)
        w = sd[n].detach().double().numpy().reshape(-1) if n in BN_WEIGHTS else 1.0
        d = rel_l2(mine * w, r * w)
        yard = max(rel_l2(refs[k]["grads"][n].detach().double().numpy().reshape(-1) * w, r * w) for k in yards)
        bound = spread * yard + FLOOR
        worst = max(worst, d / bound)
        if not quiet:
            print(f"  {label} d {n}: device {d:.3g}, float32 restatements {yard:.3g}, bound {bound:.3g}")
        if not d <= bound:
            bad.append(("gradient bound", f"{label}: d {n}: {d:.3g} > {spread} x {yard:.3g} + {FLOOR:g}"))
        if not plain <= 1e-4:
            bad.append(("gradient relative L2 1e-4", f"{label}: d {n}: relative L2 {plain:.3g} > 1e-4"))
    return worst, bad


def fixture_conditions(rec, ref, frames, forced, label):
    """Asserted on the oracle alone: every post-BN map (bn1's and the eight layers') has rms in [0.1, 10] and a
    ReLU-on fraction in [0.2, 0.8]; the forced regime has more boxes than frames and every decoded box coordinate at
    least 1e-3 px from each validity threshold."""
    for k in ["z_stem"] + [f"z{l}" for l in range(8)]:
        z = rec[k]
        rms, on = float(z.pow(2).mean().sqrt()), float((z > 0).double().mean())
        assert 0.1 <= rms <= 10, f"fixture, not kernel: {label}: post-BN map {k} has rms {rms:.3g}"
        assert 0.2 <= on <= 0.8, f"fixture, not kernel: {label}: post-BN map {k} has ReLU-on fraction {on:.3g}"
    if forced:
        n = sum(int(d.shape[0]) for fr in ref["detections"] for d in fr)
        assert n > frames, f"fixture, not kernel: {label}: {n} boxes on {frames} frames"
        boxes = ref["boxes"].detach().numpy()
        margin = min(float(np.abs(boxes[..., q] - t).min()) for q, ts in THRESHOLDS.items() for t in ts)
        assert margin >= 1e-3, f"fixture, not kernel: {label}: a box coordinate lies {margin:.3g} px from a threshold"


# ---------------------------------------------------------------------------------------------- the scorers' references
@functools.lru_cache(maxsize=None)
def _video(regime):
    """(case, frames, calibrated state, the oracle's eval forward on the stacked windows in float64 and in the two
    float32 restatements, the float64 record)."""
    case = VIDEO_CASES[regime]
    N, T, stride = case["N"], case["T"], case["stride"]
    frames = co.synth_clips(case["seed"], 0, 0, 1, N, case["H"], case["W"])[0]
    sd = calibrated_bn_state(make_cad_model(case).state_dict(), case, case["seed"])
    return (case, frames, sd) + windows_references(sd, frames, T, stride, case["key"])


def windows_references(sd, frames, T, stride, key):
    seed, step, clip0 = key
    Wn = (frames.shape[0] - T) // stride + 1
    X = torch.stack([frames[w * stride:w * stride + T] for w in range(Wn)])
    draws = co.CadDraws.make(seed, step, clip0, Wn, T)
    runs, rec = [], {}
    with torch.no_grad():
        for dtype, rev in ((torch.float64, False), (torch.float32, False), (torch.float32, True)):
            p, bufs = _split(sd, dtype)
            runs.append(co.cad_forward(p, bufs, X.to(dtype), draws, training=False, reverse_channels=rev,
                                       record=rec if dtype == torch.float64 else None))
    return runs[0], runs[1], runs[2], rec


def scorer_tol(ref, yards, spread):
    """_check_against_oracle's per-key tolerance under the bound: atol = spread x the yardsticks' largest max-abs
    distance from ref + FLOOR, rtol = 0."""
    r64 = flat_outputs(ref)
    ys = [flat_outputs(y) for y in yards]
    return {k: dict(rtol=0.0, atol=spread * max(float(np.abs(y[k][0] - r64[k][0]).max()) if r64[k][0].size else 0.0
                                                for y in ys) + FLOOR) for k in OUT_KEYS}


def windows_as_scorer_out(fw, N, T, stride):
    """An oracle forward on stacked windows in score_video's form (every frame of the cases here lies in a window)."""
    Wn = (N - T) // stride + 1
    det = {w * stride + t: fw["detections"][w][t] for w in range(Wn) for t in range(T)}
    assert sorted(det) == list(range(N))
    return {"window_starts": torch.arange(Wn) * stride, "detections": [det[f] for f in range(N)],
            "causal_factors": list(fw["causal_factors"]), "kl_losses": torch.stack(fw["kl_losses"]),
            "adjacency_matrices": torch.stack(fw["adjacency_matrices"]),
            **{k: fw[k] for k in ("anomaly_scores", "direct_predictions", "causal_anomaly_scores")}}


# ---------------------------------------------------------------------------------------------- CPU tests
def test_state_recipe():
    """calibrated_bn_state: deterministic, the regime the issue names (running_var of order 1e4 at bn1 -- the layers
    above see a network normalised below them --, |mean| / std above 1 at layer1.1, gammas of either sign in every
    layer, two eps-regime channels per layer, num_batches_tracked non-zero), and nothing but the nine BatchNorm
    layers touched."""
    case = CLIP_CASES[1]
    base = make_cad_model(case).state_dict()
    sd = calibrated_bn_state(base, case, case["seed"])
    again = calibrated_bn_state(base, case, case["seed"])
    assert all(torch.equal(sd[k], again[k]) for k in sd)
    assert any(not torch.equal(sd[k], v) for k, v in calibrated_bn_state(base, case, case["seed"] + 1).items())
    for k, v in base.items():
        if not any(k.startswith(bn + ".") for bn in co.BN_LAYERS):
            assert torch.equal(sd[k], v), k
    for i, (bn, C) in enumerate(zip(co.BN_LAYERS, co.BN_CHANNELS)):
        g, rv, rm = sd[bn + ".weight"], sd[bn + ".running_var"], sd[bn + ".running_mean"]
        assert g.shape == (C,) and g.dtype == torch.float32 and rv.dtype == torch.float32
        neg = float((g < 0).float().mean())
        assert 0.05 <= neg <= 0.5, (bn, neg)
        assert int((rv == 1e-7).sum()) == 2, bn
        assert int(sd[bn + ".num_batches_tracked"]) == 1000 + i
        assert float(sd[bn + ".bias"].abs().max()) > 0
        live = rv > 1e-6
        ratio = float((rm[live].abs() / rv[live].sqrt()).median())
        print(f"{bn}: median running_var {float(rv[live].median()):.3g}, median |mean| / std {ratio:.3g}, "
              f"negative gammas {neg:.2f}")
    assert float(sd["backbone.bn1.running_var"].median()) > 1e3
    assert float((sd["backbone.layer1.1.running_mean"].abs() / sd["backbone.layer1.1.running_var"].sqrt()).median()) > 1


@pytest.mark.parametrize("name", CLIP_IDS)
def test_clip_fixture_conditions(name):
    case, x, draws, sd = _clip_inputs(name)
    masks, pins, rec, refs = _cpu_clip_references(name)
    fixture_conditions(rec, refs["ref"]["out"], case["B"] * case["T"], case["forced"], name)
    if case["frozen"]:  # the min arm: a negative bn1 gamma whose pooled channel is not dead
        g1 = sd["backbone.bn1.weight"]
        assert int((g1 < 0).sum()) >= 2, "fixture, not kernel: the frozen stem's min arm needs negative bn1 gammas"
        assert bool((rec["pool"][:, g1 < 0] > 0).any()), "fixture, not kernel: every min-arm channel is dead"


@pytest.mark.parametrize("regime", list(VIDEO_CASES))
def test_video_fixture_conditions(regime):
    case, frames, sd, ref, a1, a2, rec = _video(regime)
    Wn = (case["N"] - case["T"]) // case["stride"] + 1
    fixture_conditions(rec, ref, Wn * case["T"], case["forced"], case["name"])
    nmax = [z.shape[0] for z in ref["causal_factors"]]
    if case["forced"]:
        assert len(set(nmax)) >= 2, f"fixture, not kernel: every window of the oracle has Nmax {nmax[0]}"
    else:
        assert nmax == [1] * Wn


@pytest.mark.parametrize("name", CLIP_IDS)
def test_references_stay_inside_the_bounds(name):
    """The bound applied to the references alone, at spread 2.0: pinned to the float64 forward's own decisions, each
    float32 restatement plays the device against the other as the only yardstick and satisfies every assertion the
    GPU clip test makes (folded statistics, counts, outputs, gradients).  Prints how far the restatements use up the
    suite's rtol 1e-4 / atol 1e-5.  Worst ratio to the bound over the five cases: 0.34-0.58."""
    case, x, draws, sd = _clip_inputs(name)
    masks, pins, rec, refs = _cpu_clip_references(name)
    for dev, yard in (("a1", "a2"), ("a2", "a1")):
        d = restatement_as_device(refs[dev], case["frozen"])
        ulp, bad = check_fold(d["fold"], sd, f"{name} {dev}")
        worst, bad2 = check_eval_clip(d, refs, (yard,), 2.0, f"{name}: {dev} against {yard}", case["frozen"], sd)
        print(f"{name}: {dev} against {yard}: worst ratio to the bound {worst:.3g}, folded statistics {ulp:.3g} ulp")
        assert not bad + bad2, "; ".join(t for _, t in bad + bad2)


@pytest.mark.parametrize("regime", list(VIDEO_CASES))
def test_scorer_references_stay_inside_the_bounds(regime):
    """The same for the scorers' comparison: each float32 restatement of the stacked windows, in score_video's form,
    passes _check_against_oracle under the bound taken from the other one at spread 2.0."""
    case, frames, sd, ref, a1, a2, rec = _video(regime)
    N, T, stride = case["N"], case["T"], case["stride"]
    r64, f1, f2 = flat_outputs(ref), flat_outputs(a1), flat_outputs(a2)
    for k in OUT_KEYS:
        print(f"{case['name']} {k}: float32 restatements {max(np.abs(f[k][0] - r64[k][0]).max() for f in (f1, f2)):.3g}"
              f" from the float64 oracle; old tolerance used "
              f"{max(old_tolerance_used(f[k][0], r64[k][0]) for f in (f1, f2)):.3g}")
    for dev, yard in ((a1, a2), (a2, a1)):
        _check_against_oracle(windows_as_scorer_out(dev, N, T, stride), ref, N, T, stride,
                              tol=scorer_tol(ref, (yard,), 2.0))


@pytest.mark.parametrize("kind", co.EVAL_BN_FAULTS)
def test_injected_faults_are_caught(kind):
    """Teeth: the float32 restatement with one fault of EVAL_BN_FAULTS injected at bn1, at a BatchNorm behind a
    stride-1 conv and at one behind a stride-2 conv plays the device and must fail at least one assertion the GPU
    tests make (folded statistics, counts, outputs, gradient bound, gradient relative L2), with both float32
    restatements as the yardstick at F32_SPREAD.  gamma_sign_in_stem is a fault of the frozen fused stem: bn1 only, on
    the frozen case.  Prints which assertions catch it (the file header has the table)."""
    name = "forced_64_frozen" if kind == "gamma_sign_in_stem" else "forced_64"
    case, x, draws, sd = _clip_inputs(name)
    masks, pins, rec, refs = _cpu_clip_references(name)
    missed = []
    for bn in ((0,) if kind == "gamma_sign_in_stem" else FAULT_BNS):
        f = restatement_as_device(eval_run(sd, x, draws, masks, pins, dtype=torch.float32, eval_fault=(kind, bn)),
                                  case["frozen"])
        _, bad = check_fold(f["fold"], sd, name)
        _, bad2 = check_eval_clip(f, refs, ("a1", "a2"), F32_SPREAD, name, case["frozen"], sd, quiet=True)
        caught = sorted({a.split(" ")[0] if a.startswith("output") else a for a, _ in bad + bad2})
        print(f"{kind} at BatchNorm {bn} ({name}): caught by {caught}")
        if not caught:
            missed.append((kind, bn))
    assert not missed, f"faults the bound let through: {missed}"


# ---------------------------------------------------------------------------------------------- GPU tests
def _frozen(m):
    for n, p in m.named_parameters():
        if n.startswith(co.FROZEN_PREFIXES):
            p.requires_grad = False
    return m


def _model(case, sd):
    m = make_cad_model(case)
    m.load_state_dict(sd)
    if case["frozen"]:
        _frozen(m)
    return m.cuda().eval()


def _assert_bn_state_unchanged(m, sd):
    now = m.state_dict()
    for bn in co.BN_LAYERS:
        for s in (".running_mean", ".running_var", ".num_batches_tracked"):
            assert torch.equal(now[bn + s].cpu(), sd[bn + s]), f"{bn + s} changed in eval mode"


def _device_fold(eng):
    from tests.golden_util import read_debug
    fold = []
    for i, C in enumerate(co.BN_CHANNELS):
        st = read_debug(eng._last[0], "stats", i)
        assert st.size == 7 * C
        fold.append(tuple(st[j * C:(j + 1) * C].copy() for j in range(4)))
    return fold


def _device_clip(case, x, sd):
    """model(x) and user_loss's backward on the device: (module, restatement_as_device's form, masks, pins)."""
    from tests.golden_util import hip_relu_masks, hip_stem_pins, reshape_masks
    B, T, H, W = x.shape[0], x.shape[1], x.shape[3], x.shape[4]
    m = _model(case, sd)
    out = m(x.cuda())
    user_loss(out, COEF.cuda()).backward()
    torch.cuda.synchronize()
    eng = m.engine()
    assert eng.stem_grad_on == (not case["frozen"])
    masks = reshape_masks(hip_relu_masks(eng, B * T), x)
    pins = hip_stem_pins(eng, B * T, H, W) if eng.stem_grad_on else None
    dev = dict(out=flat_outputs(out), fold=_device_fold(eng),
               grads={n: (None if p.grad is None else p.grad.detach().cpu().double().numpy().reshape(-1))
                      for n, p in m.named_parameters()})
    return m, dev, masks, pins


@pytest.mark.gpu
@pytest.mark.parametrize("frozen", [False, True], ids=["stem_trains", "stem_frozen"])
def test_folded_statistics_layer_by_layer(frozen):
    """One eval forward through the engine; the four forward slots of the seven-slot stats of all nine layers against
    the float64 formula on the loaded state, 1 float32 ulp per entry (the kernel forms them in double and rounds
    once), with the stem training (conv1 + bn_finalize from row-major partials) and frozen (the fused stem).
    Device run (64x64): 0.5 ulp in both variants (0.904 while the kernel took eps as a float)."""
    case, x, draws, sd = _clip_inputs("forced_64_frozen" if frozen else "forced_64")
    m = _model(case, sd)
    eng = m.engine()
    eng.forward(x.cuda(), False, 0, 0, 0)
    torch.cuda.synchronize()
    ulp, bad = check_fold(_device_fold(eng), sd, case["name"])
    print(f"{case['name']}: folded statistics at most {ulp:.3g} ulp from the float64 formula")
    assert not bad, "; ".join(t for _, t in bad)
    _assert_bn_state_unchanged(m, sd)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CLIP_IDS)
def test_eval_clip_forward_backward(name):
    """model(x) and the backward of a user loss over scores, probabilities, KL terms and detections in eval mode under
    the calibrated state: counts, every output and every gradient tensor (the pre-BN conv biases, conv1's bias and
    every BatchNorm weight and bias among them: all live in eval mode) against the float64 oracle pinned to the
    device's ReLU and pooling decisions, within F32_SPREAD x the float32 restatements' distance + 1e-6, the gradients
    within relative L2 1e-4 too.
    Device run, worst ratio to the bound (folded statistics 0.5 ulp in all): fallback_64 0.401, forced_64 0.858,
    fallback_24x40 0.558, forced_24x40 0.367, forced_64_frozen 0.698."""
    case, x, draws, sd = _clip_inputs(name)
    m, dev, masks, pins = _device_clip(case, x, sd)
    refs = clip_references(sd, x, draws, masks, pins)
    live = {n for n, g in refs["ref"]["grads"].items() if g is not None and float(g.abs().max()) > 0}
    stem = set() if case["frozen"] else {"backbone.conv1.bias", "backbone.bn1.weight", "backbone.bn1.bias"}
    assert stem | {f"{c}.bias" for c in co.BN_CONVS[1:]} | {f"{b}.{s}" for b in co.BN_LAYERS[1:]
                                                            for s in ("weight", "bias")} <= live
    ulp, bad = check_fold(dev["fold"], sd, name)
    worst, bad2 = check_eval_clip(dev, refs, ("a1", "a2"), F32_SPREAD, name, case["frozen"], sd)
    print(f"{name}: worst device ratio to the bound {worst:.3g}, folded statistics {ulp:.3g} ulp")
    assert not bad + bad2, "; ".join(t for _, t in bad + bad2)
    _assert_bn_state_unchanged(m, sd)


def _scorer_check(out, regime):
    case, frames, sd0, ref, a1, a2, rec = _video(regime)
    yards = (a1, a2)
    tol = scorer_tol(ref, yards, F32_SPREAD)
    got = {"kl_losses": list(out["kl_losses"]), "adjacency_matrices": list(out["adjacency_matrices"]),
           "detections": [out["detections"]], **{k: out[k] for k in OUT_KEYS if k not in (
               "kl_losses", "adjacency_matrices", "detections")}}
    N, T, stride = case["N"], case["T"], case["stride"]
    nmax = _check_against_oracle(out, ref, N, T, stride, tol=tol)
    # (the worst ratio to the bound, for the record; the detections of a window's frames are compared above)
    f, r = flat_outputs(got), flat_outputs(ref)
    worst = max(float(np.abs(f[k][0] - r[k][0]).max()) / tol[k]["atol"] for k in OUT_KEYS
                if k != "detections" and r[k][0].size)
    return nmax, worst


def _push_all(s, frames, sizes):
    outs, f = [], 0
    for k in sizes:
        outs.append(s.push(frames[f:f + k]))
        f += k
    assert f == frames.shape[0]
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("regime", list(VIDEO_CASES))
def test_score_video_stream_and_group(regime):
    """score_video, a live stream pushed past one full turn of its ring and a group of two streams at different
    states of progress under the calibrated state, each through test_score_video_gpu's _check_against_oracle against
    the oracle's eval forward on the stacked windows, under the bound.  fallback: N = 11, T = 4, stride 1, chunks of 4,
    64x64, the stem training; forced: N = 13, T = 5, stride 2, chunks of 6, 96x80, the stem frozen (the fused stem's
    min arm).  Scorer and clip path still agree within 1e-6; eval leaves the BatchNorm state alone.
    Device run, worst ratio to the bound: fallback 0.0675, forced 0.0785 (score_video, stream and group alike)."""
    from tests.test_stream_gpu import _concat
    case, frames, sd, r64, a1, a2, rec = _video(regime)
    N, T, stride, chunk = case["N"], case["T"], case["stride"], case["chunk"]
    seed, step, clip0 = case["key"]
    m = _model(case, sd)
    dev = frames.cuda()
    out = m.score_video(dev, window=T, stride=stride, chunk=chunk, seed=seed, step=step, clip0=clip0)
    want_nmax = [z.shape[0] for z in r64["causal_factors"]]
    nmax, w_video = _scorer_check(out, regime)
    assert nmax == want_nmax
    # live stream: ring of T + max_push - 1 < N slots, so the pushes go past one full turn
    K = 3
    s = m.open_stream(window=T, stride=stride, max_push=K, seed=seed, step=step, clip0=clip0)
    assert s.cap < N
    sizes = [K] * (N // K) + ([N % K] if N % K else [])
    nmax, w_stream = _scorer_check(_concat(_push_all(s, dev, sizes)), regime)
    assert nmax == want_nmax and s.frames_seen == N > s.cap
    # group: stream 0 runs ahead of stream 1 (other frames order: the same video from frame 0, pushed later)
    g = m.open_stream_group(2, window=T, stride=stride, max_push=K, seed=seed, step=step, clip0=(clip0, clip0))
    at, outs = [0, 0], [[], []]
    plan = [(K, 0), (K, 1), (K, 2)]
    while min(at) < N:
        ks = plan.pop(0) if plan else (K, K)
        ks = tuple(min(k, N - a) for k, a in zip(ks, at))
        res = g.push([dev[a:a + k] if k else None for a, k in zip(at, ks)])
        for i, k in enumerate(ks):
            if k:
                outs[i].append(res[i])
            at[i] += k
    w_group = 0.0
    for i in range(2):
        nmax, w = _scorer_check(_concat(outs[i]), regime)
        assert nmax == want_nmax
        w_group = max(w_group, w)
    print(f"{case['name']}: worst ratio to the bound: score_video {w_video:.3g}, stream {w_stream:.3g}, group "
          f"{w_group:.3g}")
    # scorer and clip path on the same device (stride = T windows are the clips of m(X))
    nc = N // T
    with torch.no_grad():
        clip = m(dev[:nc * T].view(nc, T, 1, case["H"], case["W"]), seed=seed, step=step, clip0=clip0)
    sv = m.score_video(dev[:nc * T], window=T, stride=T, seed=seed, step=step, clip0=clip0)
    for k in ("anomaly_scores", "direct_predictions", "causal_anomaly_scores"):
        assert float((sv[k] - clip[k]).abs().max()) <= 1e-6, k
    for k in ("kl_losses", "adjacency_matrices"):
        assert float((sv[k] - torch.stack(clip[k])).abs().max()) <= 1e-6, k
    for b in range(nc):
        assert float((sv["causal_factors"][b] - clip["causal_factors"][b]).abs().max()) <= 1e-6
        for t in range(T):
            a, c = sv["detections"][b * T + t], clip["detections"][b][t]
            assert a.shape == c.shape and (a.numel() == 0 or float((a - c).abs().max()) <= 1e-6)
    _assert_bn_state_unchanged(m, sd)


@pytest.mark.gpu
def test_eval_leaves_the_state_alone():
    """Clip forward and backward, score_video, stream pushes and a group push on one module: running_mean,
    running_var and num_batches_tracked of all nine layers stay bit-identical to what was loaded."""
    case, x, draws, sd = _clip_inputs("forced_64")
    m, dev, masks, pins = _device_clip(case, x, sd)
    frames = x.reshape(-1, 1, case["H"], case["W"]).cuda()
    m.score_video(frames, window=4, stride=1, chunk=3)
    s = m.open_stream(window=4, stride=1, max_push=2)
    _push_all(s, frames, [2, 2, 2, 2])
    g = m.open_stream_group(2, window=4, stride=1, max_push=2)
    g.push([frames[:2], frames[2:3]])
    g.push([frames[2:4], frames[3:5]])
    torch.cuda.synchronize()
    _assert_bn_state_unchanged(m, sd)


@pytest.mark.gpu
def test_state_loaded_late():
    """The module runs one eval forward and one score_video in the constructor state (the engine, its plans, weight
    images and folded statistics exist), then load_state_dict brings the calibrated state into the same module: the
    next clip forward + backward, score_video and stream pushes match the oracle under the NEW state within the
    bounds of the tests above.  A stream open across the load follows it, as stream.py promises ("a weight change
    makes later frames use the new weights"): frames pushed before keep their cached results, and every window made
    of frames pushed after the load equals the oracle's under the new state."""
    from tests.golden_util import hip_relu_masks, hip_stem_pins, reshape_masks
    from tests.test_stream_gpu import _concat
    case, x, draws, sd = _clip_inputs("fallback_64")
    vcase, frames, vsd, r64, a1, a2, rec = _video("fallback")
    B, T, H, W = case["B"], case["T"], case["H"], case["W"]
    N, Tw, stride = vcase["N"], vcase["T"], vcase["stride"]
    seed, step, clip0 = vcase["key"]
    dev = frames.cuda()
    m = make_cad_model(case).cuda().eval()
    with torch.no_grad():
        before = m(x.cuda())["direct_predictions"].clone()
    m.score_video(dev, window=Tw, stride=stride, chunk=vcase["chunk"], seed=seed, step=step, clip0=clip0)
    s = m.open_stream(window=Tw, stride=stride, max_push=3, seed=seed, step=step, clip0=clip0)
    s.push(dev[:3])
    s.push(dev[3:5])  # 5 frames, 2 windows under the constructor state
    # the video's state differs from the clip's only in the BatchNorm layers' seed; load the clip case's for the clip
    m.load_state_dict({k: v.cuda() for k, v in sd.items()})
    out = m(x.cuda())
    assert float((out["direct_predictions"].detach() - before).abs().max()) > 1e-3  # (the new state is in use)
    user_loss(out, COEF.cuda()).backward()
    torch.cuda.synchronize()
    eng = m.engine()
    masks = reshape_masks(hip_relu_masks(eng, B * T), x)
    pins = hip_stem_pins(eng, B * T, H, W)
    d = dict(out=flat_outputs(out), fold=_device_fold(eng),
             grads={n: (None if p.grad is None else p.grad.detach().cpu().double().numpy().reshape(-1))
                    for n, p in m.named_parameters()})
    refs = clip_references(sd, x, draws, masks, pins)
    ulp, bad = check_fold(d["fold"], sd, "late load")
    worst, bad2 = check_eval_clip(d, refs, ("a1", "a2"), F32_SPREAD, "late load", False, sd, quiet=True)
    assert not bad + bad2, "; ".join(t for _, t in bad + bad2)
    # score_video and the stream under the new state: the oracle on the video's frames with the loaded state
    ref, b1, b2, _ = windows_references(sd, frames, Tw, stride, vcase["key"])
    tol = scorer_tol(ref, (b1, b2), F32_SPREAD)
    sv = m.score_video(dev, window=Tw, stride=stride, chunk=vcase["chunk"], seed=seed, step=step, clip0=clip0)
    _check_against_oracle(sv, ref, N, Tw, stride, tol=tol)
    fresh = m.open_stream(window=Tw, stride=stride, max_push=3, seed=seed, step=step, clip0=clip0)
    _check_against_oracle(_concat(_push_all(fresh, dev, [3, 3, 3, 2])), ref, N, Tw, stride, tol=tol)
    # the stream opened before the load follows: frames 5.. run under the new state; the windows that start at
    # frame >= 5 hold only such frames
    late = _concat([s.push(dev[5:8]), s.push(dev[8:11])])
    starts = late["window_starts"].tolist()
    assert starts == list(range(2, 8)) and s.frames_seen == N
    for i, w in enumerate(starts):
        if w < 5:
            continue
        for k in ("anomaly_scores", "direct_predictions", "causal_anomaly_scores", "kl_losses",
                  "adjacency_matrices"):
            want = (torch.stack(ref[k]) if isinstance(ref[k], list) else ref[k])[w].numpy()
            np.testing.assert_allclose(late[k][i].cpu().numpy(), want, err_msg=f"window {w}: {k}", **tol[k])
        np.testing.assert_allclose(late["causal_factors"][i].cpu().numpy(), ref["causal_factors"][w].numpy(),
                                   **tol["causal_factors"])
    for f in range(5, N):  # the frames pushed after the load: detections under the new state
        t = min(f, Tw - 1)
        np.testing.assert_allclose(late["detections"][f - 5].cpu().numpy(), ref["detections"][f - t][t].numpy(),
                                   **tol["detections"])
    _assert_bn_state_unchanged(m, sd)
