"""The bbox clip scorer (csrc/bbox_plan.hip) stage by stage against the float64 oracle, across shapes and regimes.

Kernels: bbox_conv1_pool_kernel (conv1 + bias + ReLU + MaxPool3d(2), fp32 FMA chains), conv3d_x3_fwd as conv2 (split
bf16, three planes), adaptive_avgpool3d_fwd with its ReLU on load (both kernels), three dense_fwd calls and
bbox_tail_kernel; and, under the knob bbox_im2col = 1, im2col3d + dense_fwd + maxpool3d_fwd.  The stage tensors are read
through vad_bbox_debug_buffer (pooled, y2, hc, logits, hcl) and the outputs (features, adj, scores); the head alone runs
through vad_bbox_head_forward.  Reference: oracle.bbox_oracle.bbox_stages and its stage_* parts in float64.

Judging.  Per tensor, dist(a, r) = max |a - r| / rms(r); the device passes where
    dist(dev, r64) <= min(1e-4, max(K * d32, 1e-6)),  d32 = dist(float32 oracle, r64),  K = 6
(a reference that is all zero must be met exactly).  y2 has a second yardstick of its own, the same formula on
dist2(a, r) = rms(a - r) / rms(r) with K_L2 = 4.5: a conv2 that drops its third bf16 plane errs by 2 - 2.5e-6 of the
map's rms everywhere, where the float32 oracle's rms error is 0.5 - 2.8e-7 but its LARGEST error, over up to 260 k
sums of 864 terms, is 1 - 2.2e-6 -- on the max-norm the lost plane is 3 - 10 x d32 and passes K = 8 on the large maps,
on the rms it is 8 - 36 x d32 and above the 1e-6 floor in every case.  The float32 oracle sums the score's 128 terms
as bbox_tail_kernel does (bias first, ascending; stage_z(serial=True)), so that d32 carries what that order costs.
Every stage is judged twice: down the whole chain from x, and
locally -- r64 and the float32 oracle's d32 being the one stage applied to the device's OWN previous-stage tensor (y2
from the device's pooled, features from its y2, hc and hcl from its features, logits from its hc, adj / scores from its
logits / hcl), so that rounding collected down the chain cannot pay for a loss inside one kernel.  pooled's only input
is x, its two judgements coincide; the same formula holds it to K * d32 (a few 1e-6), far under 1e-4.  On the im2col
path the GEMM epilogue has applied conv2's ReLU to the stored y2; it is compared with relu(y2).  Outputs and the
workspace are prefilled with NaN and everything read back is finite; a 256-float guard behind each output is untouched.

Shapes (B, T, H, W), the smallest that reach each arm (test_dispatch_table restates the rules of conv3d_x3_fwd and
adaptive_avgpool3d_fwd):
  (1, 2, 2, 2)     pooled 1x1x1    conv2 <4,8,8>   per-output pool   all padding; 16 bins of one voxel
  (2, 3, 7, 6)     pooled 1x3x3    conv2 <4,8,8>   per-output        odd T floors; bins overlap (3 -> 4)
  (5, 4, 10, 10)   pooled 2x5x5    conv2 <4,8,8>   per-output        B D = 10 frames against NI = 4
  (2, 4, 17, 33)   pooled 2x8x16   conv2 <2,8,16>  per-output        whole tiles; the last odd pixel row / column is
                                                                     read as a neighbour, never pooled
  (1, 10, 40, 26)  pooled 5x20x13  conv2 <2,8,16>  block-per-bin     H > 8, odd frame count against NI = 2, ragged bins
  (3, 5, 18, 34)   pooled 2x9x17   conv2 <1,8,32>  per-output        one-voxel second tile row and column in conv1
  (1, 8, 64, 64)   pooled 4x32x32  conv2 <1,8,32>  block-per-bin     the workload's own tile
Clips: oracle.bbox_oracle.synth_clips(seed 70 + the shape's index).

Regimes, each at every shape: "default", the reference initialisation (torch seed 77), where every head
pre-activation is within a few hundredths of zero; and "o1" (generator seed 505 on top of it): encoder.0.weight x 3
(conv1 pre-activations of rms 0.7 - 1.1) with bias uniform in (-0.6, -0.1), encoder.3.weight x 3 (y2 of rms 0.4 - 1.8)
with bias uniform in (-0.5, 0.5), causal_net.0 / causal_net.2 / classifier.0 / classifier.3 weights x 6 / 4 / 6 / 12
with biases uniform in (-0.5, 0.5): logits of rms 1.7 - 6.3 (largest 5 - 24), score pre-activations in -6.4 ... 0.2.
test_fixture_conditions asserts on the float64
oracle that under o1 30 - 70 % of y2 is negative and 5 - 50 % of pooled is exactly 0 (the ReLU closed in all eight
voxels of the window).

Head seam (test_head_seam_rows): B in {1, 2, 63, 64, 65, 257} (dense_fwd's row-tile edges; split-K is chosen by M), o1
parameters, rows of kinds cycling from row 0: all zero; default scale (|N(0, 1)| x 0.05); signed N(0, 1) rows scaled
(by a fixed-point iteration on the float64 oracle) so that the row's largest |logit| is 30, 88, 90, 110, or its score
pre-activation z is +-30, +-88, +-90, +-110.  float32 exp overflows above 88.72 and 1 / (1 + exp(z)) is a denormal
float32 from 87.34 on: at 88 expf is finite and the result a denormal, at 90 and 110 expf is +inf and the result must be
exactly 0 (1 on the other side).  hc, logits, hcl: the bound above.  adj and scores: against the float64 sigmoid of the
device's own logits / z (z restated from its own hcl in the kernel's float32 order): |err| < 1e-6, no NaN, exactly
0 / 1 where |pre-activation| > 104 (below the smallest denormal's half).  The seam equals vad_bbox_forward bit for bit
on that
call's own features (test_bbox_stages, every shape, regime and path), and a second run is bit-identical.

Non-finite input (test_nan_pixel): one NaN pixel in clip 0 at an even (t, y, x) whose pooled neighbour lies across a
bin boundary of the average pool in x, in y, or (t) only in the pooled depth: torch poisons the 2 x 2 x 2 pooled voxels
whose windows touch the 3 x 3 x 3 cube of NaN conv outputs; a maximum taken with fmaxf (which returns its non-NaN
operand) poisons only the one window that lies wholly inside the cube.  The NaN masks of pooled, features, adj and
scores equal the float64 oracle's on both paths, finite entries stay inside the bound.  Oracle fault "pool_fmax"
restates the fmaxf maximum; test_fixture_conditions asserts that its masks differ from torch's at every position
(pooled) and at the x and y positions (features).  Through the seam a NaN feature in one row gives that row NaN scores
and adjacency and leaves every other row bit-identical.

Host-only self-check (test_float32_oracle_passes_and_faults_fail): the float32 oracle passes every case (d32 < 1e-4
asserted); each fault of oracle.bbox_oracle.FAULTS, run in float32 in place of the device (chain and local judgement),
fails on the cases named in FAULT_CASES.

Measured on an MI355X, one run of every case, both paths, all inside the bound.  Worst device dist / d32 per stage over
the tensors whose d32 is above the floor's share (chain | local), and the worst dist / bound of the stage:
  pooled    1.64 | -      0.27  ((1, 2, 2, 2) o1)           logits  1.20 | 1.09   0.19
  y2        2.90 | 2.93   0.49  ((1, 10, 40, 26) default)   hcl     0.86 | 0.61   0.14
  y2 (rms)  1.74 | 2.06   0.41  ((1, 8, 64, 64))            adj     1.16 | 1.00   0.19
  features  2.05 | 1.15   0.34  ((5, 4, 10, 10) default)    scores  2.86 | 1.05   0.48  ((5, 4, 10, 10) o1, im2col)
  hc        1.07 | 0.62   0.18
K: the heads' 8 leaves 2.7 x over the worst ratio (2.93, y2's largest element); 6 is the smallest whole factor with 2 x
(5.86), kept.  K_L2: 2 x 2.06 = 4.1, kept at 4.5; a lost plane's rms error is 1.3 - 2.5e-6 of the map's rms.  Before
the float32 oracle summed the score serially, local scores stood at 10.4 x d32
((2, 4, 17, 33) o1, im2col path: 1.9e-6 of the rms, an absolute 7e-8 -- the 128-term float32 sum of terms that cancel,
against torch's blocked dot product on two clips); with the kernel's order in the yardstick it is 1.05.  Seam: adj and
scores within 8.8e-8 of the float64 sigmoid of their own pre-activations.  With fmaxf in bbox_conv1_pool_kernel all six
test_nan_pixel cases failed on the fused path (32 NaN pooled values where torch has 256; features 128 against 256 / 192,
64 against 128) and passed on the im2col path; with the fix all pass.  Faults (float32, on the CPU): pad_clamp every
case, 9 judgements, 1e5 x the bound; pool_ceil the two odd-T shapes (shape mismatch); w_two_planes / act_two_planes
every case through y2 (rms), 1.3 - 2.5 x the bound, and on the max-norm only at the small maps; relu_after_avg every
o1 case but (1, 2, 2, 2) (one-voxel bins: asserted identical); bin_end_floor the five
shapes with ragged bins; no_b3 every case; tail_short every case but those whose last hidden unit is closed in every
clip (asserted identical there), tail_half every case.  The whole file runs in 5 s.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import bbox_oracle as bo

gpu = pytest.mark.gpu  # per test: the host-only checks live in this file too

K = 6.0              # every tensor, on the max-norm distance
K_L2 = {"y2": 4.5}   # conv2's output also on the rms distance (see the docstring)
FLOOR, CAP = 1e-6, 1e-4
GUARD = 256

SHAPES = [(1, 2, 2, 2), (2, 3, 7, 6), (5, 4, 10, 10), (2, 4, 17, 33), (1, 10, 40, 26), (3, 5, 18, 34), (1, 8, 64, 64)]
# shape -> (pooled D, H, W; conv2 tile <NI, TH, TW>; average-pool kernel)
DISPATCH = {
    (1, 2, 2, 2): ((1, 1, 1), (4, 8, 8), "per-output"),
    (2, 3, 7, 6): ((1, 3, 3), (4, 8, 8), "per-output"),
    (5, 4, 10, 10): ((2, 5, 5), (4, 8, 8), "per-output"),
    (2, 4, 17, 33): ((2, 8, 16), (2, 8, 16), "per-output"),
    (1, 10, 40, 26): ((5, 20, 13), (2, 8, 16), "block-per-bin"),
    (3, 5, 18, 34): ((2, 9, 17), (1, 8, 32), "per-output"),
    (1, 8, 64, 64): ((4, 32, 32), (1, 8, 32), "block-per-bin"),
}
REGIMES = ("default", "o1")
STAGES = ("pooled", "y2", "features", "hc", "logits", "hcl", "adj", "scores")
HEAD_STAGES = ("hc", "logits", "hcl")
SHAPE_IDS = ["x".join(map(str, s)) for s in SHAPES]
ODD_T = [s for s in SHAPES if s[1] % 2]
RAGGED_BINS = [s for s in SHAPES if DISPATCH[s][0][1] % 4 or DISPATCH[s][0][2] % 4]
ALL = [(s, r) for s in SHAPES for r in REGIMES]
# fault -> the (shape, regime) cases on which it has to land outside the bound
FAULT_CASES = {
    "pad_clamp": ALL,
    "pool_ceil": [(s, r) for s in ODD_T for r in REGIMES],
    "w_two_planes": ALL,
    "act_two_planes": ALL,
    "relu_after_avg": [(s, "o1") for s in SHAPES[1:]],  # (1, 2, 2, 2): every bin is the one voxel, see RELU_BLIND
    "bin_end_floor": [(s, r) for s in RAGGED_BINS for r in REGIMES],
    "no_b3": ALL,
    "tail_short": ALL,   # but for the cases where the ReLU closed the last unit in every clip: asserted blind there
    "tail_half": ALL,    # the nearest fault that lands everywhere
}
# one NaN pixel (clip 0, channel 1) at (t, y, x): see the docstring
NAN_CASES = {
    ((2, 4, 17, 33), "x"): (2, 4, 10), ((2, 4, 17, 33), "y"): (2, 6, 4), ((2, 4, 17, 33), "t"): (2, 4, 4),
    ((1, 8, 64, 64), "x"): (2, 4, 18), ((1, 8, 64, 64), "y"): (2, 18, 4), ((1, 8, 64, 64), "t"): (4, 4, 4),
}
RELU_BLIND = ((1, 2, 2, 2), "o1")
SEAM_B = (1, 2, 63, 64, 65, 257)
ROW_KINDS = ("zero", "default") + tuple(("logit", t) for t in (30, 88, 90, 110)) + tuple(
    ("z", s * t) for t in (30, 88, 90, 110) for s in (1, -1))


# ---------------------------------------------------------------------------------------------------- fixtures
def conv2_tile(D, H, W):
    """conv3d_x3_fwd's choice of <NI, TH, TW> for a pooled map"""
    if H <= 8 and W <= 8:
        return (4, 8, 8)
    return (2, 8, 16) if W <= 16 else (1, 8, 32)


def avg_kernel(D, H, W, bins=(1, 4, 4)):
    """adaptive_avgpool3d_fwd's choice of kernel"""
    return "block-per-bin" if D * H * W >= 64 * bins[0] * bins[1] * bins[2] else "per-output"


@functools.lru_cache(maxsize=None)
def _params(regime):
    """float32 parameters by state_dict name"""
    from vad_amd.bbox import CausalAnomalyDetector
    torch.manual_seed(77)
    p = {k: v.detach().clone() for k, v in CausalAnomalyDetector().state_dict().items()}
    if regime == "o1":
        g = torch.Generator().manual_seed(505)
        u = lambda n, lo, hi: torch.rand(n, generator=g) * (hi - lo) + lo
        for name, scale, lo, hi in (("encoder.0", 3.0, -0.6, -0.1), ("encoder.3", 3.0, -0.5, 0.5),
                                    ("causal_net.0", 6.0, -0.5, 0.5), ("causal_net.2", 4.0, -0.5, 0.5),
                                    ("classifier.0", 6.0, -0.5, 0.5), ("classifier.3", 12.0, -0.5, 0.5)):
            p[name + ".weight"] = p[name + ".weight"] * scale
            p[name + ".bias"] = u(p[name + ".bias"].numel(), lo, hi)
    return p


def _cast(p, dtype):
    return {k: v.to(dtype) for k, v in p.items()}


@functools.lru_cache(maxsize=None)
def _x(shape, nan_at=None):
    x = bo.synth_clips(70 + SHAPES.index(shape), 0, 0, *shape)
    if nan_at is not None:
        t, y, xx = nan_at
        x[0, 1, t, y, xx] = float("nan")
    return x


def _np(r):
    return {k: v.detach().double().numpy() for k, v in r.items()}


@functools.lru_cache(maxsize=None)
def _ref(shape, regime, dtype, fault=None, nan_at=None):
    """bbox_stages from x in `dtype` as float64 arrays (computed once, shared, never modified)"""
    with torch.no_grad():
        return _np(bo.bbox_stages(_cast(_params(regime), dtype), _x(shape, nan_at).to(dtype), fault,
                                  serial_tail=dtype == torch.float32))


def _local(regime, got, dtype, relu_y2=False):
    """Every stage in `dtype` applied to the previous-stage tensor of `got` (float64 arrays in the device's layouts)."""
    p = _cast(_params(regime), dtype)
    t = lambda name: torch.from_numpy(np.ascontiguousarray(got[name])).to(dtype)
    B = got["features"].shape[0]
    with torch.no_grad():
        y2 = bo.stage_y2(p, bo.from_ndhwc(t("pooled")))
        r = dict(y2=bo.to_ndhwc(torch.relu(y2) if relu_y2 else y2),
                 features=bo.stage_features(bo.from_ndhwc(t("y2"))),
                 hc=bo.stage_hc(p, t("features")), logits=bo.stage_logits(p, t("hc")),
                 hcl=bo.stage_hcl(p, t("features")), adj=torch.sigmoid(t("logits")).view(B, 16, 16),
                 scores=torch.sigmoid(bo.stage_z(p, t("hcl"), serial=dtype == torch.float32)))
    return _np(r)


def _dist(a, ref, l2=False):
    """max |a - ref| / rms(ref) -- l2: rms(a - ref) / rms(ref) -- over the entries where ref is finite (inf on a shape
    mismatch or a NaN in a there)"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    if a.shape != ref.shape:
        return float("inf")
    m = np.isfinite(ref)
    a, ref = a[m], ref[m]
    if a.size == 0:
        return 0.0
    if not np.isfinite(a).all():
        return float("inf")
    rms = float(np.sqrt(np.mean(np.square(ref))))
    err = float(np.sqrt(np.mean(np.square(a - ref)))) if l2 else float(np.abs(a - ref).max())
    if rms == 0:
        return 0.0 if err == 0 else float("inf")
    return err / rms


def _judge(label, got, r64, r32, names, verbose=True):
    """The tensors `names` of got under the bound.  Returns (failures, {name: (dist, d32, bound)})."""
    fails, figs = [], {}
    for name, l2 in [(n, False) for n in names] + [(n, True) for n in names if n in K_L2]:
        d32 = _dist(r32[name], r64[name], l2)
        assert d32 < CAP, (label, name, d32)  # the float32 oracle itself passes the bound
        bound = min(CAP, max((K_L2[name] if l2 else K) * d32, FLOOR))
        d = _dist(got[name], r64[name], l2)
        name = name + "/l2" if l2 else name
        figs[name] = (d, d32, bound)
        if verbose:
            print(f"[bbox] {label} {name}: dist {d:.3e} d32 {d32:.3e} dist/d32 {d / d32 if d32 else float('nan'):.2f} "
                  f"bound {bound:.3e}")
        if not d <= bound:
            fails.append(f"{label} {name}: dist {d:.3e} > bound {bound:.3e} (d32 {d32:.3e})")
    return fails, figs


def _judge_both(label, got, shape, regime, relu_y2=False, nan_at=None, verbose=True):
    """Chain and local judgement of a full set of stage tensors (float64 arrays in the device's layouts)."""
    r64, r32 = _ref(shape, regime, torch.float64, None, nan_at), _ref(shape, regime, torch.float32, None, nan_at)
    if relu_y2:
        r64, r32 = dict(r64, y2=np.maximum(r64["y2"], 0)), dict(r32, y2=np.maximum(r32["y2"], 0))
    fails, chain = _judge(label + " chain", got, r64, r32, STAGES, verbose)
    if all(got[n].shape == r64[n].shape for n in STAGES):
        f2, local = _judge(label + " local", got, _local(regime, got, torch.float64, relu_y2),
                           _local(regime, got, torch.float32, relu_y2), STAGES[1:], verbose)
        fails += f2
    else:
        local = {}
    return fails, chain, local


# ---------------------------------------------------------------------------------------------------- host only
def test_dispatch_table():
    """Each shape reaches the conv2 tile and the average-pool kernel its row of the table names."""
    for (B, T, H, W), (pooled, tile, kern) in DISPATCH.items():
        assert (T // 2, H // 2, W // 2) == pooled
        assert conv2_tile(*pooled) == tile and avg_kernel(*pooled) == kern, (B, T, H, W)
        assert B <= 5
    assert {d[1] for d in DISPATCH.values()} == {(4, 8, 8), (2, 8, 16), (1, 8, 32)}
    assert {d[2] for d in DISPATCH.values()} == {"per-output", "block-per-bin"}
    assert avg_kernel(2, 16, 32) == "block-per-bin" and avg_kernel(1, 31, 33) == "per-output"  # 1024 is the threshold


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_fixture_conditions(shape):
    r = _ref(shape, "o1", torch.float64)
    neg, closed = float((r["y2"] < 0).mean()), float((r["pooled"] == 0).mean())
    print(f"[bbox] {shape} o1: {neg:.1%} of y2 negative, {closed:.1%} of pooled exactly 0; max |logit| "
          f"{np.abs(r['logits']).max():.2f}, z {np.round(r['z'].ravel(), 2)}")
    assert 0.30 <= neg <= 0.70 and 0.05 <= closed <= 0.50
    for (s, axis), at in NAN_CASES.items():
        if s != shape:
            continue
        assert all(c % 2 == 0 for c in at)
        a, b = _ref(s, "o1", torch.float64, None, at), _ref(s, "o1", torch.float64, "pool_fmax", at)
        assert int(np.isnan(a["pooled"]).sum()) == 8 * 32 and int(np.isnan(b["pooled"]).sum()) == 32
        fa, fb = np.isnan(a["features"]), np.isnan(b["features"])
        assert fb.any() and not (fb & ~fa).any()
        assert (axis == "t") == np.array_equal(fa, fb), axis


def test_oracle_parts_are_torch():
    """The staged forward is torch's functional ops in both dtypes: composed, it is the plain forward bit for bit; the
    bin-by-bin average (which carries the bin_end_floor fault) is F.adaptive_avg_pool3d; layouts are NDHWC."""
    import torch.nn.functional as F
    for dt in (torch.float32, torch.float64):
        for shape in SHAPES[:4]:
            p, x = _cast(_params("o1"), dt), _x(shape).to(dt)
            with torch.no_grad():
                r = bo.bbox_stages(p, x)
                h = F.relu(F.conv3d(x, p["encoder.0.weight"], p["encoder.0.bias"], stride=1, padding=1))
                pooled = F.max_pool3d(h, 2)
                y2 = F.conv3d(pooled, p["encoder.3.weight"], p["encoder.3.bias"], stride=1, padding=1)
                f = F.adaptive_avg_pool3d(F.relu(y2), (1, 4, 4)).reshape(shape[0], -1)
                hc = F.relu(F.linear(f, p["causal_net.0.weight"], p["causal_net.0.bias"]))
                logits = F.linear(hc, p["causal_net.2.weight"], p["causal_net.2.bias"])
                hcl = F.relu(F.linear(f, p["classifier.0.weight"], p["classifier.0.bias"]))
                z = F.linear(hcl, p["classifier.3.weight"], p["classifier.3.bias"])
                want = dict(pooled=pooled.permute(0, 2, 3, 4, 1), y2=y2.permute(0, 2, 3, 4, 1), features=f, hc=hc,
                            logits=logits, hcl=hcl, z=z, adj=torch.sigmoid(logits).view(-1, 16, 16),
                            scores=torch.sigmoid(z))
                assert set(want) == set(r)
                for k, v in want.items():
                    assert r[k].dtype == dt and torch.equal(r[k], v), (dt, shape, k)
                s, adj, feats = bo.bbox_forward(p, x)
                assert torch.equal(s, r["scores"].squeeze()) and torch.equal(adj, r["adj"]) and torch.equal(feats, f)
                mine = bo.adaptive_avg_144(F.relu(y2)).reshape(shape[0], -1)
                assert float((mine - f).abs().max()) <= 8 * torch.finfo(dt).eps * float(f.abs().max())
    assert bo.avg_bins(3) == [(0, 1), (0, 2), (1, 3), (2, 3)] and bo.avg_bins(13)[1] == (3, 7)
    assert bo.avg_bins(3, end_floor=True) == [(0, 0), (0, 1), (1, 2), (2, 3)]


def test_float32_oracle_passes_and_faults_fail():
    """The float32 oracle is inside the bound at every case, chain and local (d32 < 1e-4 is asserted inside _judge);
    every fault, run in float32 in the device's place, is outside it on the cases named for it."""
    for shape, regime in ALL:
        fails, _, _ = _judge_both(f"float32 {shape} {regime}", _ref(shape, regime, torch.float32), shape, regime,
                                  verbose=False)
        assert not fails, fails
    for fault, cases in FAULT_CASES.items():
        for shape, regime in cases:
            bad = _ref(shape, regime, torch.float32, fault)
            if fault == "tail_short" and not _ref(shape, regime, torch.float64)["hcl"][:, -1].any():
                clean = _ref(shape, regime, torch.float32)
                assert all(np.array_equal(clean[k], bad[k]) for k in clean), (shape, regime)
                print(f"[bbox] fault tail_short on {shape} {regime}: blind, the last hidden unit is closed in every clip")
                continue
            fails, chain, local = _judge_both(f"{fault} {shape} {regime}", bad, shape, regime, verbose=False)
            worst = max((d / b, n, w) for w, figs in (("chain", chain), ("local", local))
                        for n, (d, _, b) in figs.items())
            print(f"[bbox] fault {fault} on {shape} {regime}: {len(fails)} judgements outside, worst dist/bound "
                  f"{worst[0]:.3g} ({worst[2]} {worst[1]})")
            assert fails, (fault, shape, regime)
    # a bin of one voxel averages nothing: ReLU before or after is the same function there, bit for bit
    a, b = _ref(*RELU_BLIND, torch.float32), _ref(*RELU_BLIND, torch.float32, "relu_after_avg")
    assert all(np.array_equal(a[k], b[k]) for k in a)
    a, b = _ref(SHAPES[3], "o1", torch.float32), _ref(SHAPES[3], "o1", torch.float32, "pool_fmax")
    assert all(np.array_equal(a[k], b[k]) for k in a)  # the identity on finite input


# ---------------------------------------------------------------------------------------------------- device
class _Plan:
    """A bound plan on buffers the test owns; the workspace is NaN."""

    def __init__(self, B, T, H, W, params_by_name):
        from vad_amd import _native as nat
        self.nat, self.L, self.shape = nat, nat.lib(), (B, T, H, W)
        L, dev = self.L, torch.device("cuda:0")
        self.dev = dev
        flat = torch.zeros(L.vad_bbox_param_floats())
        names = [L.vad_bbox_slot_name(i).decode() for i in range(L.vad_bbox_num_slots())]
        assert names == list(params_by_name)
        for i, n in enumerate(names):
            off, numel = L.vad_bbox_slot_offset(i), L.vad_bbox_slot_numel(i)
            assert numel == params_by_name[n].numel()
            flat[off:off + numel] = params_by_name[n].reshape(-1)
        self.params = flat.to(dev)
        self.h = ctypes.c_void_p()
        nat.check(L.vad_bbox_create(B, T, H, W, ctypes.byref(self.h)))
        nb = int(L.vad_bbox_workspace_bytes(self.h))
        assert 0 < nb < 1 << 30
        self.nws = (nb + 3) // 4
        self.ws = torch.full((self.nws + GUARD,), float("nan"), device=dev)
        assert self.ws.data_ptr() % 256 == 0
        nat.check(L.vad_bbox_bind(self.h, self.ws.data_ptr(), self.params.data_ptr()))
        self.sizes = dict(pooled=(B, T // 2, H // 2, W // 2, 32), y2=(B, T // 2, H // 2, W // 2, 64), hc=(B, 256),
                          logits=(B, 256), hcl=(B, 128))

    def close(self):
        torch.cuda.synchronize()
        self.L.vad_bbox_destroy(self.h)
        self.h = None

    def _outs(self, with_features):
        B = self.shape[0]
        o = {"scores": (B, 1), "adj": (B, 16, 16)}
        if with_features:
            o["features"] = (B, 1024)
        return {k: (torch.full((int(np.prod(s)) + GUARD,), float("nan"), device=self.dev), s) for k, s in o.items()}

    def _collect(self, outs, names):
        torch.cuda.synchronize()
        res = {}
        for k, (t, s) in outs.items():
            n = int(np.prod(s))
            assert torch.isnan(t[n:]).all(), f"the guard behind {k} was written"
            res[k] = t[:n].reshape(s).cpu()
        assert torch.isnan(self.ws[self.nws:]).all(), "the guard behind the workspace was written"
        for name in names:
            p, k = ctypes.c_void_p(), ctypes.c_int64()
            self.nat.check(self.L.vad_bbox_debug_buffer(self.h, name.encode(), ctypes.byref(p), ctypes.byref(k)))
            assert k.value == int(np.prod(self.sizes[name])), name
            off = (p.value - self.ws.data_ptr()) // 4
            assert 0 <= off and off + k.value <= self.nws, name
            res[name] = self.ws[off:off + k.value].reshape(self.sizes[name]).cpu()
        return res

    def forward(self, x, im2col):
        """vad_bbox_forward under the knob bbox_im2col -> every stage tensor, float32 on the host"""
        xd = x.contiguous().to(self.dev)
        outs = self._outs(True)
        self.nat.check(self.L.vad_set_tuning(b"bbox_im2col", im2col))
        try:
            self.nat.check(self.L.vad_bbox_forward(self.h, xd.data_ptr(), outs["scores"][0].data_ptr(),
                                                   outs["adj"][0].data_ptr(), outs["features"][0].data_ptr(),
                                                   self.nat.stream_of(self.dev)))
        finally:
            self.nat.check(self.L.vad_set_tuning(b"bbox_im2col", 0))
        return self._collect(outs, ("pooled", "y2") + HEAD_STAGES)

    def head(self, feats):
        """vad_bbox_head_forward on feature rows (B, 1024); hc, logits and hcl refilled with NaN first"""
        fd = feats.contiguous().to(self.dev)
        self.ws[:self.nws].fill_(float("nan"))
        outs = self._outs(False)
        self.nat.check(self.L.vad_bbox_head_forward(self.h, fd.data_ptr(), outs["scores"][0].data_ptr(),
                                                    outs["adj"][0].data_ptr(), self.nat.stream_of(self.dev)))
        return self._collect(outs, HEAD_STAGES)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _f64(res):
    return {k: v.double().numpy() for k, v in res.items()}


@gpu
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_bbox_stages(shape, regime):
    """Both paths, every stage, chain and local; the seam on the call's own features returns the same bits."""
    P = _Plan(*shape, _params(regime))
    try:
        fails = []
        for im2col in (0, 1):
            res = P.forward(_x(shape), im2col)
            for k, v in res.items():
                assert torch.isfinite(v).all(), f"path {im2col} {k}: non-finite"
            fails += _judge_both(f"{shape} {regime} path {im2col}", _f64(res), shape, regime, relu_y2=bool(im2col))[0]
            seam = P.head(res["features"])
            for k, v in seam.items():
                assert _bits_equal(v, res[k]), f"path {im2col} {k}: the seam differs from vad_bbox_forward"
        assert not fails, fails
    finally:
        P.close()


@functools.lru_cache(maxsize=None)
def _seam_rows(B):
    """(feature rows (B, 1024) float32, the kind of every row)"""
    p64 = _cast(_params("o1"), torch.float64)
    g = torch.Generator().manual_seed(900 + B)
    kinds = [ROW_KINDS[i % len(ROW_KINDS)] for i in range(B)]
    rows = []
    for kind in kinds:
        base = torch.randn(1024, generator=g, dtype=torch.float64)
        if kind == "zero":
            rows.append(torch.zeros(1024, dtype=torch.float64))
        elif kind == "default":
            rows.append(base.abs() * 0.05)
        else:
            what, target = kind
            alpha = 1.0
            for _ in range(60):
                for _ in range(40):
                    r = bo.bbox_head_stages(p64, (alpha * base)[None])
                    v = float(r["logits"].abs().max()) if what == "logit" else float(r["z"])
                    alpha *= abs(target) / max(abs(v), 1e-3)
                if what == "logit" or v * target > 0:
                    break
                base = torch.randn(1024, generator=g, dtype=torch.float64)  # z of the wrong sign: another direction
                alpha = 1.0
            rows.append(alpha * base)
    return torch.stack(rows).float(), kinds


@pytest.mark.parametrize("B", SEAM_B)
def test_seam_rows_reach_their_targets(B):
    """The float64 oracle on the float32 rows: every scaled row's largest |logit| / z is within 1 % of its target."""
    rows, kinds = _seam_rows(B)
    with torch.no_grad():
        r = bo.bbox_head_stages(_cast(_params("o1"), torch.float64), rows.double())
    for i, kind in enumerate(kinds):
        if kind == "zero":
            assert not rows[i].any()
        elif kind != "default":
            v = float(r["logits"][i].abs().max()) if kind[0] == "logit" else float(r["z"][i])
            want = abs(kind[1]) if kind[0] == "logit" else kind[1]
            assert abs(v - want) <= 0.01 * abs(want), (i, kind, v)
            if kind[0] == "logit":  # both signs at half the target at least
                assert float(r["logits"][i].max()) > 0.5 * want and float(r["logits"][i].min()) < -0.5 * want


def _head_checks(label, res, rows, regime="o1"):
    """The seam's tensors on rows: hc, logits, hcl under the bound (chain and local), adj and scores against the
    float64 sigmoid of the device's own pre-activations."""
    got = _f64(res)
    got["features"] = rows.double().numpy()
    with torch.no_grad():
        r64 = _np(bo.bbox_head_stages(_cast(_params(regime), torch.float64), rows.double()))
        r32 = _np(bo.bbox_head_stages(_cast(_params(regime), torch.float32), rows))
    fails, _ = _judge(label + " chain", got, r64, r32, HEAD_STAGES)
    loc = {}
    for dt in (torch.float64, torch.float32):
        p = _cast(_params(regime), dt)
        with torch.no_grad():
            loc[dt] = _np(dict(logits=bo.stage_logits(p, torch.from_numpy(got["hc"]).to(dt))))
    fails += _judge(label + " local", got, loc[torch.float64], loc[torch.float32], ("logits",))[0]
    # the device's own z is not handed out: it is restated from its hcl in the kernel's own float32 order (the bias,
    # then 128 rounded products ascending), so that this comparison holds expf and the division, not the sum -- on the
    # scaled rows the terms are in the hundreds and the sum's float32 rounding alone moves a mid-range score by 1e-6
    with torch.no_grad():
        z = bo.stage_z(_cast(_params(regime), torch.float32), res["hcl"], serial=True).double().numpy()
    for name, pre in (("adj", got["logits"].reshape(got["adj"].shape)), ("scores", z.reshape(got["scores"].shape))):
        want = 1.0 / (1.0 + np.exp(-pre))
        assert not np.isnan(got[name]).any(), f"{label} {name}: NaN"
        err = float(np.abs(got[name] - want).max())
        print(f"[bbox] {label} {name}: max |err| against the float64 sigmoid of its own pre-activation {err:.3e}; "
              f"pre-activations in [{pre.min():.1f}, {pre.max():.1f}]")
        if not err < 1e-6:
            fails.append(f"{label} {name}: |err| {err:.3e}")
        if not ((got[name][pre > 104] == 1).all() and (got[name][pre < -104] == 0).all()):
            fails.append(f"{label} {name}: not exactly 0 / 1 where expf overflows")
    return fails


@gpu
@pytest.mark.parametrize("B", SEAM_B)
def test_head_seam_rows(B):
    rows, kinds = _seam_rows(B)
    P = _Plan(B, 2, 2, 2, _params("o1"))
    try:
        res = P.head(rows)
        for k, v in res.items():
            assert torch.isfinite(v).all(), f"{k}: non-finite"
        fails = _head_checks(f"seam B={B}", res, rows)
        assert not fails, fails
        again = P.head(rows)
        for k in res:
            assert _bits_equal(res[k], again[k]), f"{k}: second run differs"
    finally:
        P.close()


@gpu
@pytest.mark.parametrize("row", (5, 64))
def test_head_seam_nan_row(row):
    """A NaN feature in one row of 65: that row's score and adjacency are NaN, every other row keeps its bits."""
    B = 65
    rows, _ = _seam_rows(B)
    rows = (rows.abs() * 0.05).clamp(max=1.0)  # moderate rows: nothing saturates
    P = _Plan(B, 2, 2, 2, _params("o1"))
    try:
        clean = P.head(rows)
        bad_rows = rows.clone()
        bad_rows[row, 517] = float("nan")
        bad = P.head(bad_rows)
        others = [i for i in range(B) if i != row]
        for k in clean:
            assert torch.isfinite(clean[k]).all(), k
            assert _bits_equal(clean[k][others], bad[k][others]), f"{k}: a clean row changed"
        assert torch.isnan(bad["scores"][row]).all() and torch.isnan(bad["adj"][row]).all()
    finally:
        P.close()


@gpu
@pytest.mark.parametrize("case", list(NAN_CASES), ids=[f"{'x'.join(map(str, s))}_{a}" for s, a in NAN_CASES])
def test_nan_pixel(case):
    """One NaN pixel: the NaN masks of pooled, features, adj and scores are the float64 oracle's on both paths, and the
    finite entries stay inside the bound."""
    shape, _ = case
    at = NAN_CASES[case]
    regime = "o1"
    r64 = _ref(shape, regime, torch.float64, None, at)
    P = _Plan(*shape, _params(regime))
    try:
        fails = []
        for im2col in (0, 1):
            res = _f64(P.forward(_x(shape, at), im2col))
            for name in ("pooled", "features", "adj", "scores"):
                want, have = np.isnan(r64[name]), np.isnan(res[name])
                print(f"[bbox] nan {shape} {at} path {im2col} {name}: {int(have.sum())} NaN on the device, "
                      f"{int(want.sum())} in the oracle")
                if not np.array_equal(want, have):
                    fails.append(f"path {im2col} {name}: NaN mask differs ({int(have.sum())} against "
                                 f"{int(want.sum())}; {int((want & ~have).sum())} missing)")
            if not fails:
                fails += _judge_both(f"nan {shape} {at} path {im2col}", res, shape, regime, relu_y2=bool(im2col),
                                     nan_at=at)[0]
        assert not fails, fails
    finally:
        P.close()
