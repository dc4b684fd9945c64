"""The a2 head and compute_improved_loss kernels alone (csrc/a2_plan.hip), against the float64 oracle, across loss
regimes.

Kernels: a2_head_fwd_clip_kernel / a2_head_fwd_kernel, a2_loss_kernel, a2_pairs_kernel, a2_loss_fin_kernel,
a2_dadj_kernel, a2_head_bwd_clip_kernel / a2_head_bwd_kernel stages 0-6, through vad_a2_head_forward /
vad_a2_head_backward: A2PlanImpl::head and ::backward_head, the functions the train step itself runs behind the average
pool, on a plan of the smallest clip (T = 1, H = W = 4; the convs never run).  test_seam_equals_step asserts that the
seam and a step agree bit for bit.  Reference: oracle.a2_oracle.a2_head + a2_loss in float64 on pooled rows built here,
gradients by autograd (the external upstream gradients applied as (out * d).sum() terms).

A fixture is: pooled rows uniform in [0, 0.5) from numpy's default_rng([fseed, case index]), the reference-init model
of torch seed 1000 + fseed (then edited), and the RNG key (seed, step, clip0) of the dropout masks and the pseudo-label
draws.  Regimes (CASES):
  edge count    causal_net.2.bias = -6 everywhere and +2 on k seeded off-diagonal entries: k edges per clip.  B = 2:
                e6, e10, e20, e40; e41 = e40 plus one entry whose weight row and bias are set (from the float64
                oracle's hc0) so that its logit is logit(0.1) + 1 in one clip and logit(0.1) - 1 in the other;
                far above: every default-regime case (240 B edges)
  pair distance default: avg 0.011 - 0.019 < 0.1 (csign -1); cs_pos: causal_net.2.weight x 60, fc.weight x 8 (csign +1)
  pseudo labels np0_mixed (0, 1), np0_none (1, 1), np0_one (B = 3, one normal clip): np = 0; found by trying key seeds
                1, 2, ... at step 0, clip0 0 with oracle.rng.uniform01 (11; 655; 64)
  ties          twin: two identical pooled rows in eval mode, every pair entry tied
  B ladder      b2, b3, b33, b64, b65, b256 at default-regime parameters (b256: pseudo-anomalous clips at indices >= 64)
  keying        key7: clip0 = 7, step = 5 (the pseudo labels differ from those of clip0 = 0)
  modes         eval5: training = 0 with the loss; every case under a2_head_clip = 1 and 0, loss-driven and module-like
                (forward without the loss, seeded external d_s, d_adj, d_f, all non-zero)
  saturation    sat0_* / sat1_*: anomaly_predictor.2.bias = -/+ 120, float32 scores exactly 0 / 1, without (_n) and
                with (_a) a pseudo-anomalous label.  The float64 chain does not saturate at -120, so only the loss stage
                is compared: the float64 a2_loss and its autograd d_s / d_adj on the device's own scores and adj.

Fixture conditions, asserted on the float64 oracle by test_fixture_conditions: every off-diagonal adj entry at least
1e-3 from 0.1; |avg - 0.1| >= 1e-3 wherever np > 0; every head ReLU pre-activation at least 1e-5 x its layer's RMS
from zero; for B <= 33 no entry of a pseudo-normal pair with 0 < |A_i - A_j| < 3e-7 (float32 adjacencies carry about
1e-7; one flipped sign moves d_adj by 5e-6 of its norm at B = 33).  From B = 64 on such near-ties are certain (about 10
of the 0.48 M pair entries at B = 64): every float32 evaluation flips its own few signs, and d32 carries them.  The
float32 oracle takes the same decisions (edges, ReLU gates, csign, pseudo; the ties for B <= 33).  fseed was found with
the oracle alone: 1, 2, ... tried in order per case, the first that meets the conditions is in CASES.

Bound per tensor: relative L2 <= min(1e-4, max(8 * d32, 1e-6)), d32 = the float32 oracle's relative L2 to the float64
oracle on the CPU; outputs (scores, adj, features) also rtol 1e-4 / atol 1e-5.  Loss words are one-element tensors.
A tensor whose reference is all zero must be exactly zero.  Exact: pseudo, edge_count, sparsity_ratio (the float32
quotient), losses[9] == 2; the diagonal of adj and of dz_cn2; with np = 0 and for the twin pair the consistency share of
d_adj is zero: every clip's d_adj is the same bits (the acyclicity share does not depend on the clip).  Outputs, saved
activations, the workspace and the fc / head slots of the gradient buffer are prefilled with NaN and what is read back
is finite; the conv slots, the slot padding, a guard behind every output and behind the workspace are untouched; a
second forward + backward is bit-identical.

Host-only self-check (test_float32_oracle_passes_and_faults_fail): the float32 oracle passes every bound (d32 < 1e-4
is asserted); each oracle fault, evaluated in float32, lands outside the bound on the cases named for it (FAULT_CASES).
struct_inclusive (the structure arms as <= 10 / >= 40) is the exception: both arms vanish at their thresholds, so it
computes the same value everywhere and no test can see it -- asserted as such; struct_shifted (arms one edge wide of the
mark) stands in for it on e10 / e40 / e41.

Measured on an MI355X, one run of every case, mode and knob value: all inside the bound.  Per case, over both modes and
both a2_head_clip values: the worst rel L2 / bound, then the worst device rel L2 / d32 over the tensors whose d32 is
above the floor's share (d32 > 1.25e-7) and the tensor that sets it:
  e6         0.31   2.5 (g1)               np0_none   0.28   1.7 (fc.bias grad)        b64    0.26   1.7 (ap.2.weight grad)
  e10        0.31   2.5 (dz_cn2)           np0_one    0.29   2.3 (g2)                  b65    0.28   1.8 (cn.0.bias grad)
  e20        0.30   2.3 (g1)               twin       0.34   2.7 (g2)                  b256   0.51   2.8 (cn.0.weight grad)
  e40        0.25   2.0 (g1)               b2         0.30   2.4 (cn.0.bias grad)      key7   0.27   2.1 (cn.2.weight grad)
  e41        0.36   2.9 (dz_cn2)           b3         0.21   1.7 (g2)                  eval5  0.24   1.7 (cn.0.bias grad)
  cs_pos     0.25   2.0 (fc.bias grad)     b33        0.22   1.8 (cn.0.bias grad)
  np0_mixed  0.25   2.0 (g1)               sat0_n / sat0_a / sat1_n / sat1_a  0.05 / 0.07 / 0.05 / 0.08 (every d32 at the floor)
so the factor 8 stands (worst 2.9).  The two knob values differ by at most 0.1 in either figure, except fc's own
gradients at cs_pos (1.1 per clip, 0.6 as GEMMs)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import a2_oracle as ao
from oracle import rng

gpu = pytest.mark.gpu  # per test: the host-only checks live in this file too

FACTOR, FLOOR, CAP = 8.0, 1e-6, 1e-4
GUARD = 256
SENT = -7.5
TIE = 3e-7
LOGIT01 = float(np.log(0.1 / 0.9))
HEAD_PREFIXES = ("feature_extractor.fc.", "causal_discovery.", "graph_encoder.", "anomaly_predictor.")
OUT_NAMES = ("scores", "adj", "features")
ACT_NAMES = ("hc0", "sig", "g1", "g1d", "g2", "cat", "hp0")                       # vad_a2_head_forward's saved[0..6]
ACT_W = (32, 256, 128, 128, 64, 80, 32)
DZ_NAMES = ("dz_ap2", "dz_ap0", "dg2", "dz_ge0", "dz_cn2", "dz_cn0", "dfeat")     # vad_a2_head_backward's dz[0..6]
DZ_OF = ("z_ap2", "z_ap0", "g2", "z_ge0", "z_cn2", "z_cn0", "f0")                 # the oracle tensor each differentiates
DZ_W = (1, 32, 64, 128, 256, 32, 16)
LOSS_NAMES = ("total", "anomaly_loss", "acyclicity_loss", "sparsity_loss", "consistency_loss", "structure_loss",
              "edge_count", "sparsity_ratio")
MODES = ("loss", "module")
OFFDIAG = np.array([e for e in range(256) if e // 16 != e % 16])

# key = (seed, step, clip0) of the draws; pseudo = the labels it gives; fseed: see the docstring
CASES = {
    "e6": dict(B=2, key=(1, 0, 0), pseudo=(0, 0), fseed=4, edges=3),
    "e10": dict(B=2, key=(1, 0, 0), pseudo=(0, 0), fseed=1, edges=5),
    "e20": dict(B=2, key=(1, 0, 0), pseudo=(0, 0), fseed=1, edges=10),
    "e40": dict(B=2, key=(1, 0, 0), pseudo=(0, 0), fseed=1, edges=20),
    "e41": dict(B=2, key=(1, 0, 0), pseudo=(0, 0), fseed=1, edges=20, split=True),
    "cs_pos": dict(B=2, key=(1, 0, 0), pseudo=(0, 0), fseed=181, scale=(60.0, 8.0)),
    "np0_mixed": dict(B=2, key=(11, 0, 0), pseudo=(0, 1), fseed=1),
    "np0_none": dict(B=2, key=(655, 0, 0), pseudo=(1, 1), fseed=1),
    "np0_one": dict(B=3, key=(64, 0, 0), pseudo=(0, 1, 1), fseed=1),
    "twin": dict(B=2, key=(1, 0, 0), pseudo=(0, 0), fseed=1, twin=True, training=0),
    "b2": dict(B=2, key=(1, 0, 0), pseudo=(0, 0), fseed=1),
    "b3": dict(B=3, key=(3, 0, 0), pseudo=(0, 0, 0), fseed=1),
    "b33": dict(B=33, key=(1, 0, 0), pseudo=None, fseed=24),
    "b64": dict(B=64, key=(1, 0, 0), pseudo=None, fseed=1),
    "b65": dict(B=65, key=(1, 0, 0), pseudo=None, fseed=1),
    "b256": dict(B=256, key=(1, 0, 0), pseudo=None, fseed=3),
    "key7": dict(B=4, key=(1, 5, 7), pseudo=(0, 0, 1, 0), fseed=1),
    "eval5": dict(B=5, key=(1, 0, 0), pseudo=None, fseed=1, training=0),
    "sat0_n": dict(B=2, key=(1, 0, 0), pseudo=(0, 0), fseed=1, sat=-120.0),
    "sat0_a": dict(B=2, key=(11, 0, 0), pseudo=(0, 1), fseed=1, sat=-120.0),
    "sat1_n": dict(B=2, key=(1, 0, 0), pseudo=(0, 0), fseed=1, sat=120.0),
    "sat1_a": dict(B=2, key=(11, 0, 0), pseudo=(0, 1), fseed=1, sat=120.0),
}
CHAIN_CASES = [c for c in CASES if "sat" not in CASES[c]]
SAT_CASES = [c for c in CASES if "sat" in CASES[c]]
EDGES = {"e6": 6, "e10": 10, "e20": 20, "e40": 40, "e41": 41}
NP0 = ("np0_mixed", "np0_none", "np0_one")
# fault -> (the cases it should show on, the modes it can show in)
FAULT_CASES = {
    "struct_shifted": (("e10", "e40", "e41"), ("loss",)),
    "pairs_twice": (("cs_pos", "b3"), ("loss",)),
    "pseudo_in_pairs": (NP0 + ("b256",), ("loss",)),
    "pseudo_no_clip0": (("key7",), ("loss",)),
    "focal_short": (("b2", "b33"), ("loss",)),
    "acyc_no_t": (("b2", "e20"), ("loss",)),
    "df_dropped": (("b3", "eval5"), ("module",)),
    "fc_drop_bwd": (("b2", "key7"), MODES),
    "diag_bwd": (("b2", "eval5"), MODES),
}


# ---------------------------------------------------------------------------------------------------- fixtures
def _init_params(fseed):
    from vad_amd.a2 import CausalAnomalyDetector
    torch.manual_seed(1000 + fseed)
    m = CausalAnomalyDetector()
    return {k: v.detach().clone() for k, v in m.state_dict().items() if k.startswith(HEAD_PREFIXES)}


@functools.lru_cache(maxsize=None)
def _fixture(cid, fseed=None):
    """Inputs of a case: float32 pooled rows (B, 4096), head parameters, the draws' key, upstream gradients."""
    c = CASES[cid]
    fseed = c["fseed"] if fseed is None else fseed
    B = c["B"]
    g = np.random.default_rng([fseed, sorted(CASES).index(cid)])
    pooled = g.uniform(0.0, 0.5, size=(B, 4096)).astype(np.float32)
    if c.get("twin"):
        pooled[1] = pooled[0]
    p = _init_params(fseed)
    seed, step, clip0 = c["key"]
    training = c.get("training", 1)
    if "edges" in c:
        sel = OFFDIAG[g.permutation(len(OFFDIAG))]
        b = torch.full((256,), -6.0)
        b[torch.from_numpy(sel[:c["edges"]])] = 2.0
        p["causal_discovery.causal_net.2.bias"] = b
        if c.get("split"):  # one more entry above 0.1 in one clip, below it in the other
            e = int(sel[c["edges"]])
            rec = {}
            with torch.no_grad():
                ao.a2_head({k: v.double() for k, v in p.items()}, torch.from_numpy(pooled).double(),
                           ao.A2Draws.make(seed, step, clip0, B), bool(training), rec)
            w = p["causal_discovery.causal_net.2.weight"]
            z = rec["hc0"] @ w[e].double()
            assert B == 2 and abs(float(z[0] - z[1])) > 1e-4, cid
            k = 2.0 / float(z[0] - z[1])
            w[e] *= k
            b[e] = LOGIT01 - k * float(z.mean())
    if "scale" in c:
        p["causal_discovery.causal_net.2.weight"] *= c["scale"][0]
        p["feature_extractor.fc.weight"] *= c["scale"][1]
    if "sat" in c:
        p["anomaly_predictor.2.bias"] = torch.full((1,), c["sat"])
    up = dict(d_s=g.uniform(-1, 1, B), d_adj=g.standard_normal((B, 16, 16)), d_f=g.standard_normal((B, 16)))
    up = {k: v.astype(np.float32) for k, v in up.items()}
    assert all((v != 0).all() for v in up.values())
    return dict(B=B, pooled=pooled, params=p, key=(seed, step, clip0), training=training, up=up)


def _n64(t, like):
    return (torch.zeros_like(like) if t is None else t).detach().double().numpy()


@functools.lru_cache(maxsize=None)
def _oracle(cid, mode, dtype, fault=None, fseed=None):
    """a2_head (+ a2_loss) and autograd in `dtype`, in the device's layouts: dict name -> float64 array, plus
    "pseudo", "np", "avg" and the record of the head."""
    f = _fixture(cid, fseed)
    B = f["B"]
    seed, step, clip0 = f["key"]
    p = {k: v.to(dtype).requires_grad_() for k, v in f["params"].items()}
    pooled = torch.from_numpy(f["pooled"]).to(dtype).requires_grad_()
    draws = ao.A2Draws.make(seed, step, clip0, B)
    if fault == "pseudo_no_clip0":
        draws.u_pseudo = ao.A2Draws.make(seed, step, 0, B).u_pseudo
    rec = {}
    s, adj, feat = ao.a2_head(p, pooled, draws, bool(f["training"]), rec, fault if fault in ao.HEAD_FAULTS else None)
    r = {"scores": s.reshape(B), "adj": adj, "features": feat}
    r.update({k: rec[k] for k in ACT_NAMES})
    info = {}
    if mode == "loss":
        lf = fault if fault in ao.LOSS_FAULTS else None
        obj, comps, pseudo = ao.a2_loss(s, adj, draws.u_pseudo, lf, info)
        r.update(_loss_stage(s, adj, draws.u_pseudo, lf))
        info["pseudo"] = pseudo.numpy().astype(np.int64)
    else:
        up = {k: torch.from_numpy(v).to(dtype) for k, v in f["up"].items()}
        obj = (s.reshape(B) * up["d_s"]).sum() + (adj * up["d_adj"]).sum()
        if fault != "df_dropped":
            obj = obj + (feat * up["d_f"]).sum()
    names = list(p)
    inter = [rec[k] for k in DZ_OF]
    gs = torch.autograd.grad(obj, [pooled] + [p[n] for n in names] + inter, allow_unused=True)
    r["dpooled"] = _n64(gs[0], pooled)
    r.update({"grad/" + n: _n64(gr, p[n]) for n, gr in zip(names, gs[1:1 + len(names)])})
    r.update({n: _n64(gr, t).reshape(B, -1) for n, gr, t in zip(DZ_NAMES, gs[1 + len(names):], inter)})
    r = {k: (v.detach().double().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}
    return r, info, rec


def _loss_stage(s, adj, u_pseudo, fault=None):
    """a2_loss on detached scores / adj: the loss words and d total / d scores, d total / d adj."""
    s_d, adj_d = s.detach().clone().requires_grad_(), adj.detach().clone().requires_grad_()
    total, comps, _ = ao.a2_loss(s_d, adj_d, u_pseudo, fault)
    ds, dadj = torch.autograd.grad(total, [s_d, adj_d], allow_unused=True)
    r = {"loss/" + k: np.array([float(total.detach()) if k == "total" else comps[k]]) for k in LOSS_NAMES}
    r["d_s"] = _n64(ds, s_d).reshape(-1)
    r["d_adj"] = _n64(dadj, adj_d)
    return r


def _rel(a, ref):
    a, ref = np.asarray(a, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    nr = np.linalg.norm(ref)
    if nr == 0:
        return 0.0 if not a.any() else float("inf")
    return float(np.linalg.norm(a - ref) / nr)


def _judge(label, got, r64, r32, verbose=True):
    """Every tensor of r64 in `got` under the bound (d32 from r32).  Returns (failures, worst rel / bound, worst rel /
    d32 over the tensors whose d32 is above the floor's share); prints every figure."""
    fails, w_bound, w_d32 = [], 0.0, (0.0, "")
    for name, ref in r64.items():
        d32 = _rel(r32[name], ref)
        assert d32 < CAP, (label, name, d32)  # the float32 oracle itself passes the bound
        bound = min(CAP, max(FACTOR * d32, FLOOR))
        rel = _rel(got[name], ref)
        w_bound = max(w_bound, rel / bound)
        if d32 > FLOOR / FACTOR:
            w_d32 = max(w_d32, (rel / d32, name))
        if verbose:
            print(f"[a2head] {label} {name}: rel {rel:.3e} d32 {d32:.3e} bound {bound:.3e}")
        if not rel <= bound:
            fails.append(f"{name}: rel L2 {rel:.3e} > bound {bound:.3e} (d32 {d32:.3e})")
        if name in OUT_NAMES and not np.allclose(got[name], ref, rtol=1e-4, atol=1e-5):
            fails.append(f"{name}: outside rtol 1e-4 / atol 1e-5")
    print(f"[a2head] {label}: worst rel/bound {w_bound:.3g}, worst rel/d32 {w_d32[0]:.3g} ({w_d32[1]})")
    return fails, w_bound, w_d32


# ---------------------------------------------------------------------------------------------------- host only
def _pair_gaps(adj, pseudo):
    """|A_i - A_j| over the off-diagonal entries of every pseudo-normal pair i < j: (n pairs, 240)."""
    a = adj.reshape(len(adj), 256)[pseudo == 0][:, OFFDIAG]
    i, j = np.triu_indices(len(a), 1)
    return np.abs(a[i] - a[j])


def _conditions(cid, fseed=None):
    """The fixture conditions of the docstring on the float64 oracle, and the float32 oracle's decisions."""
    B = CASES[cid]["B"]
    r64, i64, rec64 = _oracle(cid, "loss", torch.float64, None, fseed)
    r32, i32, rec32 = _oracle(cid, "loss", torch.float32, None, fseed)
    bad = []
    off = r64["adj"].reshape(B, 256)[:, OFFDIAG]
    if np.abs(off - 0.1).min() < 1e-3:
        bad.append(f"adj within {np.abs(off - 0.1).min():.2e} of 0.1")
    if i64["np"] > 0 and abs(i64["avg"] - 0.1) < 1e-3:
        bad.append(f"avg {i64['avg']:.5f} within 1e-3 of 0.1")
    for name in ao.HEAD_RELU_LAYERS:
        a, b = rec64[name].detach(), rec32[name].detach()
        lim = 1e-5 * float(a.pow(2).mean().sqrt())
        if float(a.abs().min()) < lim:
            bad.append(f"{name}: min |pre-activation| {float(a.abs().min()):.3e} < {lim:.3e}")
        if not torch.equal(a > 0, b > 0):
            bad.append(f"{name}: float32 decides differently")
    if not np.array_equal(r64["adj"] > 0.1, r32["adj"] > 0.1) or r64["loss/edge_count"] != r32["loss/edge_count"]:
        bad.append("edges differ in float32")
    if not np.array_equal(i64["pseudo"], i32["pseudo"]) or i64["np"] != i32["np"]:
        bad.append("pseudo differs in float32")
    if i64["np"] > 0 and (i64["avg"] > 0.1) != (i32["avg"] > 0.1):
        bad.append("csign differs in float32")
    if B <= 33 and i64["np"] > 0:
        g64, g32 = _pair_gaps(r64["adj"], i64["pseudo"]), _pair_gaps(r32["adj"], i32["pseudo"])
        near = (g64 > 0) & (g64 < TIE)
        if near.any():
            bad.append(f"{int(near.sum())} pair entries within {TIE} of a tie")
        if not np.array_equal(g64 == 0, g32 == 0):
            bad.append("ties differ in float32")
    return bad


@pytest.mark.parametrize("cid", list(CASES))
def test_fixture_conditions(cid):
    assert _conditions(cid) == []


def _pseudo_of(cid, clip0=None):
    seed, step, c0 = CASES[cid]["key"]
    u = rng.uniform01(seed, rng.S_A2_PSEUDO, step, c0 if clip0 is None else clip0, CASES[cid]["B"], 1).reshape(-1)
    return (u > np.float32(0.95)).astype(np.int64)


def test_fixtures_cover_what_they_claim():
    for cid, c in CASES.items():
        r, info, _ = _oracle(cid, "loss", torch.float64)
        ps = _pseudo_of(cid)
        assert np.array_equal(info["pseudo"], ps), cid
        if c["pseudo"] is not None:
            assert tuple(ps.tolist()) == c["pseudo"], (cid, ps)
        nn = int((ps == 0).sum())
        assert info["np"] == (nn * (nn - 1) // 2 if nn > 1 else 0), cid
        if cid in EDGES:
            assert r["loss/edge_count"][0] == EDGES[cid], (cid, r["loss/edge_count"])
        elif "sat" not in c and "scale" not in c:
            assert r["loss/edge_count"][0] == 240 * c["B"], (cid, r["loss/edge_count"])
    st = lambda cid: float(_oracle(cid, "loss", torch.float64)[0]["loss/structure_loss"][0])
    assert st("e6") == pytest.approx(0.04) and st("e41") == pytest.approx(0.01) and st("b2") == pytest.approx(4.4)
    assert st("e10") == 0 and st("e20") == 0 and st("e40") == 0
    info = lambda cid: _oracle(cid, "loss", torch.float64)[1]
    assert info("b2")["np"] == 1 and info("b2")["avg"] < 0.1 < info("cs_pos")["avg"]
    for cid in NP0:
        assert info(cid)["np"] == 0, cid
    assert _pseudo_of("np0_one").sum() == 2 and _pseudo_of("np0_none").sum() == 2 and _pseudo_of("np0_mixed").sum() == 1
    assert info("twin")["np"] == 1 and info("twin")["avg"] == 0
    assert _pseudo_of("b256")[64:].any() and info("b256")["np"] > 0
    assert not np.array_equal(_pseudo_of("key7"), _pseudo_of("key7", clip0=0))
    for cid in SAT_CASES:  # the float32 oracle saturates as the device does; at -120 the float64 one does not (7.7e-53)
        s32 = _oracle(cid, "loss", torch.float32)[0]["scores"]
        s64 = _oracle(cid, "loss", torch.float64)[0]["scores"]
        assert (s32 == (0.0 if CASES[cid]["sat"] < 0 else 1.0)).all(), cid
        assert CASES[cid]["sat"] > 0 or (s64 > 0).all(), cid


def _sat_refs(cid, scores, adj):
    """The loss stage in float64 and float32 on given float32 scores (B,) and adj (B, 16, 16)."""
    seed, step, clip0 = CASES[cid]["key"]
    u = ao.A2Draws.make(seed, step, clip0, CASES[cid]["B"]).u_pseudo
    s, a = torch.from_numpy(np.asarray(scores, np.float32)), torch.from_numpy(np.asarray(adj, np.float32))
    return _loss_stage(s.double(), a.double(), u), _loss_stage(s, a, u)


def test_float32_oracle_passes_and_faults_fail():
    """The float32 oracle is inside the bound on every case and mode (asserted inside _judge); every fault, evaluated in
    float32, is outside it on the cases named for it, in the modes it can show in."""
    for cid in CHAIN_CASES:
        for mode in MODES:
            r32 = _oracle(cid, mode, torch.float32)[0]
            fails, _, _ = _judge(f"float32 {cid}/{mode}", r32, _oracle(cid, mode, torch.float64)[0], r32, verbose=False)
            assert not fails, (cid, mode, fails)
    for cid in SAT_CASES:
        r32 = _oracle(cid, "loss", torch.float32)[0]
        ref64, ref32 = _sat_refs(cid, r32["scores"], r32["adj"])
        assert all(np.isfinite(v).all() for v in ref64.values()), cid
        fails, _, _ = _judge(f"float32 {cid}/loss stage", ref32, ref64, ref32, verbose=False)
        assert not fails, (cid, fails)
    for fault, (cids, modes) in FAULT_CASES.items():
        for cid in cids:
            for mode in modes:
                r64, r32 = _oracle(cid, mode, torch.float64)[0], _oracle(cid, mode, torch.float32)[0]
                fails, wb, _ = _judge(f"fault {fault} {cid}/{mode}", _oracle(cid, mode, torch.float32, fault)[0], r64,
                                      r32, verbose=False)
                print(f"[a2head] fault {fault} on {cid}/{mode}: {len(fails)} tensors outside, worst rel/bound "
                      f"{wb:.3g}: " + "; ".join(fails[:3]))
                assert fails, (fault, cid, mode)
    # <= 10 / >= 40: (10 - E) and (E - 40) are zero at E = 10 and E = 40, so the inclusive arms give the same value
    for cid in ("e6", "e10", "e20", "e40", "e41", "b2"):
        a, b = _oracle(cid, "loss", torch.float32)[0], _oracle(cid, "loss", torch.float32, "struct_inclusive")[0]
        assert all(np.array_equal(a[k], b[k]) for k in a), cid


# ---------------------------------------------------------------------------------------------------- device
def _slots():
    from vad_amd import _native as nat
    L = nat.lib()
    names = [L.vad_a2_slot_name(i).decode() for i in range(L.vad_a2_num_slots())]
    return {n: (L.vad_a2_slot_offset(i), L.vad_a2_slot_numel(i)) for i, n in enumerate(names)}, names


class _Plan:
    """A bound plan of the smallest clip on buffers the test owns: workspace and head gradient slots NaN, the rest of
    the gradient buffer a sentinel."""

    def __init__(self, B, params_by_name):
        from vad_amd import _native as nat
        self.nat, self.L, self.B = nat, nat.lib(), B
        L, dev = self.L, torch.device("cuda:0")
        self.dev = dev
        self.slots, names = _slots()
        self.head = [n for n in names if n.startswith(HEAD_PREFIXES)]
        assert self.head == list(params_by_name)
        nparam = L.vad_a2_param_floats()
        params = torch.zeros(nparam)
        grads = torch.full((nparam + GUARD,), SENT)
        self.mask = torch.zeros(nparam + GUARD, dtype=torch.bool)
        for n, v in params_by_name.items():
            off, numel = self.slots[n]
            assert numel == v.numel()
            params[off:off + numel] = v.reshape(-1)
            self.mask[off:off + numel] = True
        grads[self.mask] = float("nan")
        self.params, self.grads = params.to(dev), grads.to(dev)
        self.m, self.v = torch.zeros(nparam, device=dev), torch.zeros(nparam, device=dev)
        self.steps = torch.zeros(len(names), dtype=torch.int32, device=dev)
        self.h = ctypes.c_void_p()
        nat.check(L.vad_a2_create(B, 1, 4, 4, ctypes.byref(self.h)))
        nb = int(L.vad_a2_workspace_bytes(self.h))
        self.nws = (nb + 3) // 4
        self.ws = torch.full((self.nws + GUARD,), float("nan"), device=dev)
        assert self.ws.data_ptr() % 256 == 0
        nat.check(L.vad_a2_bind(self.h, self.ws.data_ptr(), *[t.data_ptr() for t in (self.params, self.grads, self.m,
                                                                                      self.v, self.steps)]))
        self.bufs = []

    def out(self, *shape):
        """A NaN-filled output with a guard behind it."""
        n = int(np.prod(shape))
        t = torch.full((n + GUARD,), float("nan"), device=self.dev)
        self.bufs.append((t, n))
        return t

    def close(self):
        torch.cuda.synchronize()
        self.L.vad_a2_destroy(self.h)
        self.h = None

    def check_untouched(self):
        for t, n in self.bufs:
            assert torch.isnan(t[n:]).all(), "a guard behind an output was written"
        assert torch.isnan(self.ws[self.nws:]).all(), "the guard behind the workspace was written"
        g = self.grads.cpu()
        assert (g[~self.mask] == SENT).all(), "a gradient outside the fc / head slots was written"
        assert torch.isfinite(g[self.mask]).all(), "a fc / head gradient slot keeps a NaN"
        return g


def _run_device(cid, mode, clip):
    """One forward (+ loss) + backward through the seam on fresh, prefilled buffers; everything copied to the host as
    float32 tensors under the oracle's names."""
    from vad_amd import _native as nat
    L = nat.lib()
    f = _fixture(cid)
    B = f["B"]
    seed, step, clip0 = f["key"]
    P = _Plan(B, f["params"])
    try:
        nat.check(L.vad_set_tuning(b"a2_head_clip", clip))
        st = nat.stream_of(P.dev)
        pooled = torch.from_numpy(f["pooled"]).to(P.dev)
        o = {"scores": P.out(B), "adj": P.out(B, 256), "features": P.out(B, 16), "losses": P.out(10),
             "pseudo": P.out(B), "d_s": P.out(B), "d_adj": P.out(B, 256), "dpooled": P.out(B, 4096)}
        o.update({k: P.out(B, w) for k, w in zip(ACT_NAMES + DZ_NAMES, ACT_W + DZ_W)})
        arr = lambda ks: (ctypes.c_void_p * len(ks))(*[o[k].data_ptr() for k in ks])
        loss = mode == "loss"
        nat.check(L.vad_a2_head_forward(P.h, pooled.data_ptr(), f["training"], seed, step, clip0, int(loss),
                                        o["scores"].data_ptr(), o["adj"].data_ptr(), o["features"].data_ptr(),
                                        o["losses"].data_ptr(), arr(ACT_NAMES + ("pseudo",)), st))
        if loss:
            nat.check(L.vad_a2_loss_grads(P.h, o["d_s"].data_ptr(), o["d_adj"].data_ptr(), st))
            ext = [None, None, None]
        else:
            up = {k: torch.from_numpy(v).to(P.dev) for k, v in f["up"].items()}
            ext = [up[k].data_ptr() for k in ("d_s", "d_adj", "d_f")]
        nat.check(L.vad_a2_head_backward(P.h, *ext, o["dpooled"].data_ptr(), arr(DZ_NAMES), st))
        torch.cuda.synchronize()
        g = P.check_untouched()
        skip = () if loss else ("losses", "pseudo", "d_s", "d_adj")
        res = {}
        for (t, n), k in zip(P.bufs, o):
            if k in skip:
                assert torch.isnan(t).all(), f"{k}: written without the loss"
                continue
            res[k] = t[:n].cpu()
            assert torch.isfinite(res[k]).all(), f"{k}: non-finite"
        for n in P.head:
            off, numel = P.slots[n]
            res["grad/" + n] = g[off:off + numel].clone()
        return res
    finally:
        L.vad_set_tuning(b"a2_head_clip", 1)
        P.close()


def _as_ref_layout(res, r64):
    got = {k: v.double().numpy().reshape(r64[k].shape) for k, v in res.items() if k in r64}
    if "losses" in res:
        for i, k in enumerate(LOSS_NAMES):
            got["loss/" + k] = res["losses"][i:i + 1].double().numpy()
    return got


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _rerun_is_identical(cid, mode, clip, res):
    r2 = _run_device(cid, mode, clip)
    for k in res:
        assert _bits_equal(res[k], r2[k]), f"{k}: second run differs"


@gpu
@pytest.mark.parametrize("clip", (1, 0))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cid", CHAIN_CASES)
def test_a2_head_matches_float64(cid, mode, clip):
    B = CASES[cid]["B"]
    res = _run_device(cid, mode, clip)
    r64, info, _ = _oracle(cid, mode, torch.float64)
    r32 = _oracle(cid, mode, torch.float32)[0]
    got = _as_ref_layout(res, r64)
    fails, _, _ = _judge(f"device {cid}/{mode}/clip{clip}", got, r64, r32)
    assert not fails, fails
    eye = np.eye(16, dtype=bool)
    assert not got["adj"][:, eye].any(), "adj diagonal"
    assert not got["dz_cn2"].reshape(B, 16, 16)[:, eye].any(), "dz_cn2 diagonal"
    if mode == "loss":
        L = res["losses"].numpy()
        assert np.array_equal(res["pseudo"].numpy().astype(np.int64), info["pseudo"]), "pseudo"
        assert L[6] == r64["loss/edge_count"][0], "edge_count"
        assert L[7] == np.float32(L[6]) / np.float32(B * 256), "sparsity_ratio"
        assert L[9] == 2.0
        if info["np"] == 0 or CASES[cid].get("twin"):  # no consistency share: d_adj does not depend on the clip
            for b in range(1, B):
                assert _bits_equal(res["d_adj"][b * 256:(b + 1) * 256], res["d_adj"][:256]), f"d_adj of clip {b}"
    _rerun_is_identical(cid, mode, clip, res)


@gpu
@pytest.mark.parametrize("clip", (1, 0))
@pytest.mark.parametrize("cid", SAT_CASES)
def test_a2_loss_stage_at_saturated_scores(cid, clip):
    """Scores exactly 0 / 1: the focal BCE's log clamp and its derivative's clamp are live.  The loss words, d_s and
    d_adj against the float64 loss evaluated on the device's own scores and adj; everything stays finite (asserted for
    every output, saved activation, scratch gradient and gradient slot in _run_device)."""
    res = _run_device(cid, "loss", clip)
    assert (res["scores"] == (0.0 if CASES[cid]["sat"] < 0 else 1.0)).all(), res["scores"]
    assert np.array_equal(res["pseudo"].numpy().astype(np.int64), _pseudo_of(cid))
    ref64, ref32 = _sat_refs(cid, res["scores"].numpy(), res["adj"].numpy().reshape(-1, 16, 16))
    got = _as_ref_layout(res, ref64)
    fails, _, _ = _judge(f"device {cid}/loss stage/clip{clip}", got, ref64, ref32)
    assert not fails, fails
    assert res["losses"][9] == 2.0
    _rerun_is_identical(cid, "loss", clip, res)


@gpu
def test_seam_equals_step():
    """A train step's forward + loss + backward at A2_CASES[0], then the seam on the plan's own pooled rows: scores,
    adj, features, the loss words and the whole gradient buffer come out bit for bit the same."""
    from tests.golden.cases import A2_CASES
    from tests.test_a2_gpu import _vad
    from vad_amd import _native as nat
    case = A2_CASES[0]
    B, T, H, W = case["B"], case["T"], case["H"], case["W"]
    vad = _vad(case)
    x = ao.synth_clips(case["seed"], case["step"], 0, B, T, H, W).cuda()
    vad.model.train()
    e = vad.model.engine(x)
    key = (case["seed"], case["step"], 0)
    e.forward(x, True, *key, with_loss=True)
    e.backward()
    torch.cuda.synchronize()
    p = e.cur
    step = [t.clone() for t in (p.scores, p.adj, p.feats, e.losses, e.grads)]
    assert all(torch.isfinite(t).all() for t in step) and float(e.losses[9]) == 2.0
    for n, o, k in e.slots:  # the seam has to write every fc / head slot again
        if n.startswith(HEAD_PREFIXES):
            e.grads[o:o + k].fill_(float("nan"))
    seam = [torch.full_like(t, float("nan")) for t in step[:4]]
    st = e.stream()
    nat.check(nat.lib().vad_a2_head_forward(p.h, None, 1, *key, 1, *[t.data_ptr() for t in seam], None, st))
    nat.check(nat.lib().vad_a2_head_backward(p.h, None, None, None, None, None, st))
    torch.cuda.synchronize()
    for name, a, b in zip(("scores", "adj", "features", "losses", "grads"), step, seam + [e.grads]):
        assert _bits_equal(a, b), name
