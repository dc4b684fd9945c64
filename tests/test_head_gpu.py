"""The causal head's kernels alone (csrc/head.hip), against the float64 oracle, across detection-count regimes.

Kernels: head_rows_fwd / head_seq_fwd (head_fwd) and head_seq_bwd / head_rows_bwd (head_bwd), head_slab_reduce,
head_rows_wgrad, through vad_head_forward / vad_head_backward (csrc/ops_api.hip), which fill HeadArgs with the function
the cad plan fills its own with (cad_head_args, csrc/cad_plan.hip).  Reference: oracle.cad_oracle.head_forward in
float64 on logits built here from a count table, gradients by autograd with the upstream gradients applied as
(out * d).sum() terms.

Cases (counts per frame, 0 = no box in range -> the fallback box; see CASES): n1_real (N = 1 with a real box), n2_t2
(m = 2, T = the BPTT chunk), mixed_t7 (fallback frames inside a live clip, a fallback-only clip beside live ones),
peak_t9 (N set by the first / the last frame only), ladder_b5t4 (N = 1..5 side by side), long_t33, t8_eval
(training = 0), clip0_7 (clip0 = 7).  Each runs with loss-like upstream gradients (d_causal, d_kl) and module-like ones
(also d_z, d_adj, d_boxes).  In-range slots are a seeded choice, not a prefix in at least one frame of every case;
out-of-range slots sit low or high in x or y (all four are used); every x and y is at least 1 px from 10 / 350 / 230 in
float64, so counts, nmax, clip_flags and the slot pattern are exact.

Bound per tensor and case: relative L2 <= min(1e-4, max(8 * d32, 1e-6)), d32 = the float32 oracle's relative L2 to the
float64 oracle on the CPU; outputs also rtol 1e-4 / atol 1e-5.  A tensor whose reference is all zero must be exactly
zero.  Exact: counts, nmax, clip_flags; z rows >= N and adj outside the off-diagonal m x m block are 0; d_det_logits is
0 at every out-of-range slot and in every fallback frame; the structure learner's gradients are 0 when no clip has
N >= 2, structure_params' always; every output and the head range of the gradient buffer are prefilled with NaN and
must be finite afterwards (so is the scratch: a row array the kernels read without having written would show); the rest
of the gradient buffer and a guard behind the scratch are untouched; a second forward + backward is bit-identical.

ReLU kinks (a condition of the fixtures): in the float64 oracle every ReLU pre-activation of the head is at least
1e-5 x its layer's RMS from zero, |cur - prd| >= 1e-5 per factor, and the float32 oracle takes the same decisions.
The seeds were found with the oracle alone (seeds 1, 2, ... tried in order per case; seed 1 met the condition for all
eight); test_fixtures_stay_clear_of_relu_kinks asserts it.  Seed s of a case gives numpy's default_rng([s, case index])
for counts, slots, logits and upstream gradients, and torch seed 1000 + s for the reference-init model: CASES.

Host-only self-check (test_float32_oracle_passes_and_faults_fail): the float32 oracle passes the bound by
construction (d32 <= max(8 d32, 1e-6); d32 < 1e-4 is asserted); each oracle fault, evaluated in float32, must land
outside the bound on each case named for it.  Measured, worst rel L2 / bound over the tensors (loss-like | module-like):
  pad_gi_zero    peak_t9 5.8e5 | 4.9e5 (58 tensors outside)
  fallback_grad  mixed_t7 4.2e4 | 3.0e5 (d_det_logits alone, rel L2 0.56 | 0.30)
  nmax_last      peak_t9 2.1e6 | 2.1e6 (nmax [1, 4], clip_flags, 61 tensors)
  kl_mean5       ladder_b5t4 6.0e5 | 9.2e4 (kl rel L2 0.49, 23 tensors)
  bptt_stop      n2_t2 4.0e5 | 2.9e5; long_t33 4.4e2 | 5.3e2 (d_det_logits, the ReID and GRU gradients: 10 tensors)
  no_compact     n2_t2 1.9e7 | 5.6e6; mixed_t7 1.0e6 | 3.7e6; ladder_b5t4 1.1e6 | 3.5e6 (counts, nmax, every tensor)

Measured on an MI355X, one run of every case and mode: all inside the bound; worst rel L2 / bound, then the worst
device rel L2 / d32 over the tensors whose d32 is above the floor's share (d32 > 1.25e-7), loss-like | module-like:
  n1_real      0.34 | 0.76    2.7 | 6.1   (tracker.reid_net.2.bias | traj_encoder.gru.bias_hh_l0)
  n2_t2        0.41 | 0.18    3.3 | 1.5
  mixed_t7     0.30 | 0.26    2.4 | 2.1
  peak_t9      0.64 | 0.64    1.8 | 1.8
  ladder_b5t4  0.20 | 0.35    1.6 | 2.2
  long_t33     0.28 | 0.23    1.3 | 1.8
  t8_eval      0.15 | 0.20    1.2 | 1.6
  clip0_7      0.31 | 0.24    2.5 | 1.9
so the factor 8 stands (worst 6.1).  Below that share the floor of 1e-6 decides: one-element tensors whose float32
oracle happens to land within 1e-9 .. 4e-8 of float64 (the scorers' last biases, edge_predictor.2.bias) sit at device
rel L2 6e-8 .. 6.4e-7, up to 110 x their d32 and at most 0.64 of the floor.  causal is within 8.4e-8 everywhere.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import cad_oracle as co

gpu = pytest.mark.gpu  # per test: the host-only checks live in this file too

RNG_SEED, RNG_STEP = 11, 5   # the (seed, step) of the VAE noise and the scorer dropout
FACTOR, FLOOR, CAP = 8.0, 1e-6, 1e-4
GUARD = 256
SENT = -7.5
HEAD_PREFIXES = ("tracker.", "traj_encoder.", "causal_extractor.", "structure_learner.", "dynamics_predictor.",
                 "anomaly_scorer.")
STRUCT_SLOTS = ("structure_learner.node_encoder.weight", "structure_learner.node_encoder.bias",
                "structure_learner.edge_predictor.0.weight", "structure_learner.edge_predictor.0.bias",
                "structure_learner.edge_predictor.2.weight", "structure_learner.edge_predictor.2.bias")
H_SP = "structure_learner.structure_params"
OUT_NAMES = ("causal", "kl", "z", "adj", "boxes")
MODES = ("loss", "module")

# counts: a table [B][T], or ("seeded", lo, hi, must) = seeded counts in lo..hi that contain every value of `must`
CASES = {
    "n1_real": dict(B=1, T=1, counts=[[1]], seed=1),
    "n2_t2": dict(B=2, T=2, counts=[[2, 1], [1, 2]], seed=1),
    "mixed_t7": dict(B=3, T=7, counts=[[0, 3, 0, 5, 1, 0, 2], [0] * 7, [1] * 7], seed=1),
    "peak_t9": dict(B=2, T=9, counts=[[4] + [1] * 8, [1] * 8 + [4]], seed=1),
    "ladder_b5t4": dict(B=5, T=4, counts=[[b + 1] * 4 for b in range(5)], seed=1),
    "long_t33": dict(B=1, T=33, counts=("seeded", 0, 5, (0, 5)), seed=1),
    "t8_eval": dict(B=2, T=8, counts=("seeded", 0, 5, ()), seed=1, training=0),
    "clip0_7": dict(B=2, T=5, counts=("seeded", 1, 5, ()), seed=1, clip0=7),
}
FAULT_CASES = {  # fault -> the cases it should show on
    "pad_gi_zero": ("peak_t9",),
    "fallback_grad": ("mixed_t7",),
    "nmax_last": ("peak_t9",),
    "kl_mean5": ("ladder_b5t4",),
    "bptt_stop": ("n2_t2", "long_t33"),
    "no_compact": ("n2_t2", "mixed_t7", "ladder_b5t4"),
}


# ---------------------------------------------------------------------------------------------------- fixtures
def _logit(v):
    return np.log(v / (1.0 - v))


@functools.lru_cache(maxsize=None)
def _fixture(cid, seed=None):
    """Inputs of a case: float32 logits (B, T, 20), the valid pattern, head parameters, upstream gradients."""
    from tests.golden_util import make_cad_model
    c = CASES[cid]
    seed = c["seed"] if seed is None else seed
    B, T = c["B"], c["T"]
    tag = sorted(CASES).index(cid)
    g = np.random.default_rng([seed, tag])
    counts = c["counts"]
    if isinstance(counts, tuple):
        _, lo, hi, must = counts
        while True:
            counts = g.integers(lo, hi + 1, size=(B, T))
            if all((counts == v).any() for v in must):
                break
    counts = np.asarray(counts, np.int64).reshape(B, T)
    valid = np.zeros((B, T, 5), bool)
    forced = False
    for b in range(B):
        for t in range(T):
            n = int(counts[b, t])
            sel = np.sort(g.choice(5, size=n, replace=False))
            if not forced and 1 <= n <= 4:  # the first frame that can: in-range slots that are no prefix
                while sel[-1] == n - 1:
                    sel = np.sort(g.choice(5, size=n, replace=False))
                forced = True
            valid[b, t, sel] = True
    logits = g.standard_normal((B, T, 5, 4))
    kinds = np.full((B, T, 5), -1)
    x = g.uniform(40.0, 320.0, size=(B, T, 5))
    y = g.uniform(30.0, 210.0, size=(B, T, 5))
    off = g.uniform(2.0, 7.0, size=(B, T, 5))
    kinds[~valid] = g.integers(0, 4, size=int((~valid).sum()))
    x = np.where(kinds == 0, off, np.where(kinds == 1, 360.0 - off, x))
    y = np.where(kinds == 2, off, np.where(kinds == 3, 240.0 - off, y))
    logits[..., 0] = _logit(x / 360.0)
    logits[..., 1] = _logit(y / 240.0)
    logits = logits.reshape(B, T, 20).astype(np.float32)
    # in float64 on the float32 logits: every x and y at least 1 px from its thresholds, validity as planned
    l4 = logits.astype(np.float64).reshape(B, T, 5, 4)
    xs, ys = 360.0 / (1.0 + np.exp(-l4[..., 0])), 240.0 / (1.0 + np.exp(-l4[..., 1]))
    assert (np.abs(xs - 10) >= 1).all() and (np.abs(xs - 350) >= 1).all()
    assert (np.abs(ys - 10) >= 1).all() and (np.abs(ys - 230) >= 1).all()
    assert (((xs > 10) & (xs < 350) & (ys > 10) & (ys < 230)) == valid).all()
    assert (np.maximum(valid.sum(-1), 1) == np.maximum(counts, 1)).all()
    nonprefix = any(valid[b, t].any() and not valid[b, t, :valid[b, t].sum()].all() for b in range(B) for t in range(T))
    assert nonprefix, cid
    m = make_cad_model(dict(seed=1000 + seed, forced=None))
    params = {k: v.detach().clone() for k, v in m.state_dict().items() if k.startswith(HEAD_PREFIXES)}
    up = dict(d_causal=g.uniform(-1, 1, B), d_kl=g.uniform(0.02, 0.2, B), d_z=g.standard_normal((B, 5, 6)),
              d_adj=g.standard_normal((B, 6, 6)), d_boxes=g.standard_normal((B, T, 5, 4)) * 0.01)
    up = {k: v.astype(np.float32) for k, v in up.items()}
    return dict(B=B, T=T, logits=logits, valid=valid, kinds=kinds, counts=np.maximum(counts, 1), params=params, up=up,
                training=c.get("training", 1), clip0=c.get("clip0", 0))


@functools.lru_cache(maxsize=None)
def _oracle(cid, mode, dtype, fault=None, seed=None):
    """head_forward and its autograd in `dtype`, in the device's layouts: (outputs, integers, gradients, record)."""
    f = _fixture(cid, seed)
    B, T = f["B"], f["T"]
    p = {k: v.to(dtype).requires_grad_() for k, v in f["params"].items()}
    lg = torch.from_numpy(f["logits"]).to(dtype).requires_grad_()
    draws = co.CadDraws.make(RNG_SEED, RNG_STEP, f["clip0"], B, T)
    rec = {}
    o = co.head_forward(p, lg, draws, training=bool(f["training"]), record=rec, fault=fault)
    up = {k: torch.from_numpy(v).to(dtype) for k, v in f["up"].items()}
    z = torch.zeros(B, 5, 6, dtype=dtype)
    boxes = torch.zeros(B, T, 5, 4, dtype=dtype)
    counts = np.zeros((B, T), np.int64)
    for b in range(B):
        z[b, :o["causal_factors"][b].shape[0]] = o["causal_factors"][b]
        for t, det in enumerate(o["detections"][b]):
            boxes[b, t, :det.shape[0]] = det
            counts[b, t] = det.shape[0]
    out = dict(causal=o["causal_anomaly_scores"].reshape(B), kl=torch.stack(o["kl_losses"]), z=z,
               adj=torch.stack(o["adjacency_matrices"]), boxes=boxes)
    loss = (out["causal"] * up["d_causal"]).sum() + (out["kl"] * up["d_kl"]).sum()
    if mode == "module":
        loss = loss + (z * up["d_z"]).sum() + (out["adj"] * up["d_adj"]).sum() + (boxes * up["d_boxes"]).sum()
    names = list(p)
    gs = torch.autograd.grad(loss, [lg] + [p[n] for n in names], allow_unused=True)
    n64 = lambda t, like: (torch.zeros_like(like) if t is None else t).detach().double().numpy()
    grads = {"d_det_logits": n64(gs[0], lg)}
    grads.update({n: n64(gr, p[n]) for n, gr in zip(names, gs[1:])})
    nmax = np.array([v.shape[0] for v in o["causal_factors"]], np.int64)
    ints = dict(counts=counts, nmax=nmax,
                clip_flags=np.stack([o["valid"].numpy().any((1, 2)).astype(np.int64), (nmax >= 2).astype(np.int64)], 1))
    return {k: v.detach().double().numpy() for k, v in out.items()}, ints, grads, rec


def _rel(a, ref):
    a, ref = np.asarray(a, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    nr = np.linalg.norm(ref)
    if nr == 0:
        return 0.0 if not a.any() else float("inf")
    return float(np.linalg.norm(a - ref) / nr)


def _judge(label, got_out, got_ints, got_grads, cid, mode, verbose=True):
    """Every tensor of `got` against the float64 oracle under the bound.  Returns (failures, worst rel / bound, worst
    rel / d32 over tensors with d32 > 0); prints every figure."""
    o64, i64, g64, _ = _oracle(cid, mode, torch.float64)
    o32, _, g32, _ = _oracle(cid, mode, torch.float32)
    fails, w_bound, w_d32 = [], 0.0, 0.0
    for k in ("counts", "nmax", "clip_flags"):
        if not np.array_equal(np.asarray(got_ints[k], np.int64), i64[k]):
            fails.append(f"{k}: {np.asarray(got_ints[k]).tolist()} != {i64[k].tolist()}")
    for kind, got, r64, r32 in (("out", got_out, o64, o32), ("grad", got_grads, g64, g32)):
        for name, ref in r64.items():
            d32 = _rel(r32[name], ref)
            assert d32 < CAP, (cid, mode, name, d32)  # the float32 oracle itself passes the bound
            bound = min(CAP, max(FACTOR * d32, FLOOR))
            rel = _rel(got[name], ref)
            w_bound = max(w_bound, rel / bound)
            if d32 > 0:
                w_d32 = max(w_d32, rel / d32)
            if verbose:
                print(f"[head] {label} {cid}/{mode} {name}: rel {rel:.3e} d32 {d32:.3e} bound {bound:.3e}")
            if not rel <= bound:
                fails.append(f"{name}: rel L2 {rel:.3e} > bound {bound:.3e} (d32 {d32:.3e})")
            if kind == "out" and not np.allclose(got[name], ref, rtol=1e-4, atol=1e-5):
                fails.append(f"{name}: outside rtol 1e-4 / atol 1e-5")
    print(f"[head] {label} {cid}/{mode}: worst rel/bound {w_bound:.3g}, worst rel/d32 {w_d32:.3g}")
    return fails, w_bound, w_d32


# ---------------------------------------------------------------------------------------------------- host only
def test_fixtures_cover_what_they_claim():
    kinds = set()
    for cid in CASES:
        f = _fixture(cid)
        kinds |= set(np.unique(f["kinds"][f["kinds"] >= 0]).tolist())
        _, ints, _, _ = _oracle(cid, "loss", torch.float64)
        assert np.array_equal(ints["counts"], f["counts"]), cid
    assert kinds == {0, 1, 2, 3}, kinds  # out of range low and high, in x and in y
    n = lambda cid: _oracle(cid, "loss", torch.float64)[1]
    assert n("n1_real")["nmax"].tolist() == [1] and n("n1_real")["clip_flags"].tolist() == [[1, 0]]
    assert n("n2_t2")["nmax"].tolist() == [2, 2]
    assert n("mixed_t7")["nmax"].tolist() == [5, 1, 1] and n("mixed_t7")["clip_flags"].tolist() == [[1, 1], [0, 0], [1, 0]]
    assert n("peak_t9")["nmax"].tolist() == [4, 4]
    assert n("ladder_b5t4")["nmax"].tolist() == [1, 2, 3, 4, 5]
    c = CASES["long_t33"]
    raw = _fixture("long_t33")["valid"].sum(-1)
    assert (raw == 0).any() and (raw == 5).any() and c["T"] == 33


@pytest.mark.parametrize("cid", list(CASES))
def test_fixtures_stay_clear_of_relu_kinks(cid):
    assert _kinks(cid) == []


def _kinks(cid, seed=None):
    _, i64, _, r64 = _oracle(cid, "loss", torch.float64, None, seed)
    _, i32, _, r32 = _oracle(cid, "loss", torch.float32, None, seed)
    bad = []
    for k in i64:
        if not np.array_equal(i64[k], i32[k]):
            bad.append(f"{k} differs in float32")
    for name in co.HEAD_RELU_LAYERS + (co.HEAD_ABS,):
        if name not in r64:
            assert name == "edge0", name  # no edges: no clip with N >= 2
            continue
        a = torch.cat([v.reshape(-1) for v in r64[name]])
        b = torch.cat([v.reshape(-1) for v in r32[name]])
        lim = 1e-5 if name == co.HEAD_ABS else 1e-5 * float(a.pow(2).mean().sqrt())
        if float(a.abs().min()) < lim:
            bad.append(f"{name}: min |pre-activation| {float(a.abs().min()):.3e} < {lim:.3e}")
        if not torch.equal(a > 0, b > 0):
            bad.append(f"{name}: float32 decides differently")
    return bad


def test_float32_oracle_passes_and_faults_fail():
    """The float32 oracle is inside the bound on every case and mode (asserted inside _judge); every fault, evaluated in
    float32, is outside it on the cases named for it."""
    for cid in CASES:
        for mode in MODES:
            o, i, g, _ = _oracle(cid, mode, torch.float32)
            fails, _, _ = _judge("float32", o, i, g, cid, mode, verbose=False)
            assert not fails, (cid, mode, fails)
    for fault, cids in FAULT_CASES.items():
        for cid in cids:
            shown = []
            for mode in MODES:
                o, i, g, _ = _oracle(cid, mode, torch.float32, fault)
                fails, wb, _ = _judge(f"fault {fault}", o, i, g, cid, mode, verbose=False)
                shown.append(bool(fails))
                print(f"[head] fault {fault} on {cid}/{mode}: {len(fails)} tensors outside, worst rel/bound {wb:.3g}: "
                      + "; ".join(fails[:3]))
            assert all(shown), (fault, cid, shown)


# ---------------------------------------------------------------------------------------------------- device
def _slots():
    from vad_amd import _native as nat
    L = nat.lib()
    names = [L.vad_cad_slot_name(i).decode() for i in range(L.vad_cad_num_slots())]
    return {n: (L.vad_cad_slot_offset(i), L.vad_cad_slot_numel(i)) for i, n in enumerate(names)}, names


def _run_device(cid, mode):
    """One forward + backward on fresh, prefilled buffers; everything copied to the host."""
    from vad_amd import _native as nat
    L = nat.lib()
    f = _fixture(cid)
    B, T = f["B"], f["T"]
    dev = torch.device("cuda:0")
    slots, names = _slots()
    head = [n for n in names if n.startswith(HEAD_PREFIXES)]
    assert head == list(f["params"]) and names.index(head[-1]) - names.index(head[0]) == len(head) - 1
    h0 = slots[head[0]][0]
    h1 = slots[names[names.index(head[-1]) + 1]][0]
    nparam = L.vad_cad_param_floats()
    params = torch.zeros(nparam)
    for n, v in f["params"].items():
        off, numel = slots[n]
        assert numel == v.numel()
        params[off:off + numel] = v.reshape(-1)
    params = params.to(dev)
    grads = torch.full((nparam + 256,), SENT, device=dev)
    grads[h0:h1] = float("nan")
    ns = L.vad_head_scratch_floats(B, T)
    assert ns > 0
    scratch = torch.full((ns + GUARD,), float("nan"), device=dev)
    fl = lambda *s: torch.full(s, float("nan"), device=dev)
    it = lambda *s: torch.full(s, -12345, dtype=torch.int32, device=dev)
    out = dict(causal=fl(B), kl=fl(B), z=fl(B, 5, 6), adj=fl(B, 6, 6), boxes=fl(B, T, 5, 4))
    ints = dict(counts=it(B, T), nmax=it(B), clip_flags=it(B, 2))
    dlog = fl(B, T, 20)
    lg = torch.from_numpy(f["logits"]).to(dev)
    up = {k: torch.from_numpy(v).to(dev) for k, v in f["up"].items()}
    ptr = lambda t: None if t is None else t.data_ptr()
    outs = [ptr(out[k]) for k in OUT_NAMES] + [ptr(ints[k]) for k in ("counts", "nmax", "clip_flags")]
    st = nat.stream_of(dev)
    key = (f["training"], RNG_SEED, RNG_STEP, f["clip0"])
    nat.check(L.vad_head_forward(ptr(lg), B, T, ptr(params), *key, *outs, ptr(scratch), ns, st))
    opt = [ptr(up[k]) if mode == "module" else None for k in ("d_z", "d_adj", "d_boxes")]
    nat.check(L.vad_head_backward(ptr(lg), B, T, ptr(params), *key, *outs, ptr(up["d_causal"]), ptr(up["d_kl"]), *opt,
                                  ptr(grads), ptr(dlog), ptr(scratch), ns, st))
    torch.cuda.synchronize()
    assert torch.isnan(scratch[ns:]).all(), "the guard behind the scratch was written"
    g = grads.cpu()
    assert (g[:h0] == SENT).all() and (g[h1:] == SENT).all(), "a gradient outside the head range was written"
    hg = {n: g[slots[n][0]:slots[n][0] + slots[n][1]].reshape(f["params"][n].shape) for n in head}
    res = dict(out={k: v.cpu() for k, v in out.items()}, ints={k: v.cpu() for k, v in ints.items()},
               grads=dict(hg, d_det_logits=dlog.cpu()), head_range=g[h0:h1].clone())
    return res


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cid", list(CASES))
def test_head_matches_float64(cid, mode):
    f = _fixture(cid)
    r = _run_device(cid, mode)
    # nothing the head owns is left unwritten
    for k, v in list(r["out"].items()) + list(r["grads"].items()):
        assert torch.isfinite(v).all(), f"{k}: non-finite"
    assert torch.isfinite(r["head_range"]).all(), "the head range of the gradient buffer keeps a NaN"
    for k, v in r["ints"].items():
        assert (v != -12345).all(), f"{k}: unwritten"
    out = {k: v.double().numpy() for k, v in r["out"].items()}
    ints = {k: v.numpy().astype(np.int64) for k, v in r["ints"].items()}
    grads = {k: v.double().numpy() for k, v in r["grads"].items()}
    fails, _, _ = _judge("device", out, ints, grads, cid, mode)
    assert not fails, fails
    # exact zeros
    nmax = ints["nmax"]
    for b in range(f["B"]):
        N = int(nmax[b])
        assert not out["z"][b, N:].any(), "z rows >= N"
        blk = np.zeros((6, 6), bool)
        blk[:N, :N] = True
        blk &= ~np.eye(6, dtype=bool)
        assert not out["adj"][b][~blk].any(), "adj outside the off-diagonal m x m block"
    dl = grads["d_det_logits"].reshape(f["B"], f["T"], 5, 4)
    assert not dl[~f["valid"]].any(), "d_det_logits at an out-of-range slot (fallback frames included)"
    if f["valid"].any():
        assert dl[f["valid"]].any()
    assert not grads[H_SP].any()
    if nmax.max() < 2:
        for n in STRUCT_SLOTS:
            assert not grads[n].any(), n
    # determinism: no atomics, fixed-order slab sums
    r2 = _run_device(cid, mode)
    for grp in ("out", "ints", "grads"):
        for k in r[grp]:
            a, b = r[grp][k].contiguous(), r2[grp][k].contiguous()
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{k}: second run differs"
