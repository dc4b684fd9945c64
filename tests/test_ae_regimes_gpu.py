"""The cad1 memory autoencoder against float64 across clip-count regimes, layer by layer.

The 64x64 frames have no ragged edges: what can go wrong in csrc/ae_plan.hip and csrc/conv4.hip is a function of B
(clips after the normal-label filter) and T.  REGIMES reaches what the whole-model tests never did: B = 1 (BN groups of
16 values, 16-row GEMMs), BN row tiles that go partial with more than one tile per group (Mg = 320, 272), T > 16 (the
second and third pass of the 16-group loops of gbn_finalize_kernel / gbn_bwd_finalize_kernel, with their chained
running stats), T = 1 in training, and rings at the fill boundary 9 / 10, filled exactly to the end and wrapping in
mid-batch.  test_table_reaches_its_regimes restates that arithmetic.

Method (tests/test_grad64.py's): one train step on the device through AeTrainer.step, on both conv paths (ae_direct
1 / 0), against the float64 oracle step pinned to the device's own LeakyReLU decisions (golden_util.ae_leaky_pins),
tensor by tensor so that a failure names its layer: the raw conv outputs, the BN batch statistics, the decoder
Linear, the LSTM's per-step input projection / gates / cell state and the BPTT's d gates (vad_ae_debug_buffer), the
outputs, the loss, every gradient, the seven BNs' running stats and counters, the ring and the parameters after Adam.
Eval mode runs at the same shapes with non-default running statistics, forward and module autograd.

Tolerances.  Outputs: test_ae_gpu's rtol 1e-4 / atol 1e-5.  Gradients: relative L2 <= 1e-4 (test_grad64.TOL); the
pre-BN conv biases (true gradient exactly zero) at noise level.  Intermediates and running stats: 2x the float32 CPU
oracle's own relative-L2 distance from float64 on the same case and pins, at least 1e-4 (test_grad64's derived
bound).  Parameters after Adam: test_optim_gpu's bound and method -- float64 Adam on the gradient the
device's optimizer was given, 2x the float32 restatement's distance from it + one ulp of the tensor's largest value
(against the float64 step's own gradient, elements with |g| near Adam's eps move by 1e5 x the gradient's rounding).
The ring and its pointer are exact against ae_oracle.update_memory on the device's own sequence features.

Measured float32-oracle distances from float64 (relative L2, worst over the six cases, this file's CPU test prints
them per case): ey 6.6e-7, dy 9.8e-7, est 3.3e-7, dst 4.0e-7, u 7.4e-7, lat 8.8e-7, gx 8.6e-7, gates 2.3e-7,
cs 8.0e-7, seq 7.5e-7, dG 1.4e-6 (b2t17), running stats 9.1e-7 (b2t33), gradients 2.4e-6.  Every derived bound
therefore sits on its 1e-4 floor; no case needed more, b1t1's BN over 16 values included (est 3.3e-7 there).  On
an MI355X all six cases pass on both conv paths inside these bounds.

The memory kernels alone (vad_ae_update_memory / vad_ae_memory_score): exact ring writes at every wrap position
with NaN features, and scores at the fill levels around the 10-row threshold and the 256-thread stride, with zero
rows, zero features, cos clamped at +-1 and NaN in the feature and in the nearest ring row.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import ae_oracle as ae
from oracle.mc_oracle import adam_update
from tests.test_ae_oracle import PRE_BN_BIASES, make_ae_model

TOL = 1e-4  # test_grad64.TOL: pinned gradients, and the floor of its derived bounds
LR = 1e-3   # one Adam step moves every element by ~lr: far above float32 rounding of the parameters
MEM, R_TILE = 500, 256

REGIMES = [
    dict(name="b1t1", B=1, T=1, seed=71, ptr=9),     # fewer than 10 rows: score 0
    dict(name="b1t2", B=1, T=2, seed=72, ptr=10),    # the first real score
    dict(name="b5t3", B=5, T=3, seed=73, ptr=495),   # ptr + B = 500: the pointer returns to 0
    dict(name="b17t1", B=17, T=1, seed=74, ptr=490),  # wraps in mid-batch: rows 490..499, 0..6
    dict(name="b2t17", B=2, T=17, seed=75, ptr=499),  # wraps after one row
    dict(name="b2t33", B=2, T=33, seed=76, ptr=257),  # one row past the 256-thread stride of the score loop
]
IDS = [r["name"] for r in REGIMES]
ENC = ((1, 32, 32), (32, 64, 16), (64, 128, 8), (128, 128, 4))  # Ci, Co, output size
DEC = ((128, 128, 8), (128, 64, 16), (64, 32, 32))
INTERMEDIATE = ("ey", "est", "dy", "dst", "u", "lat", "gx", "gates", "cs", "seq", "dG")


def _rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


class Case:
    """One regime: clips, fresh parameters, and a fully populated ring whose row at the write pointer is clip 0's own
    sequence feature -- a score that reads one row too many finds it, and the first row the step overwrites is the
    nearest one."""

    def __init__(self, r):
        self.name, self.B, self.T, self.seed, self.ptr = r["name"], r["B"], r["T"], r["seed"], r["ptr"]
        self.x = ae.synth_clips(self.seed, 0, 0, self.B, self.T)
        self.spec = dict(name=self.name, B=self.B, T=self.T, seed=self.seed, lr=LR, mem=None)
        self.params, self.bufs, _ = ae.split_state(make_ae_model(self.spec).state_dict())
        ring = np.random.default_rng(self.seed).standard_normal((MEM, 64)).astype(np.float32)
        with torch.no_grad():
            seq = ae.ae_forward(_cast(self.params, torch.float64), _cast(self.bufs, torch.float64), self.x.double(),
                                True)["sequence_feature"]
        ring[self.ptr] = seq[0].numpy().astype(np.float32)
        self.ring = torch.from_numpy(ring)

    def model(self, bufs=None):
        m = make_ae_model(self.spec)
        with torch.no_grad():
            m.normal_memory.copy_(self.ring)
            m.memory_ptr.fill_(self.ptr)
            if bufs is not None:
                m.load_state_dict(bufs, strict=False)
        return m


@functools.lru_cache(maxsize=None)
def case_of(name):
    return Case(next(r for r in REGIMES if r["name"] == name))


def _cast(d, dtype):
    return {k: v.detach().to(dtype).clone() for k, v in d.items()}


# ------------------------------------------------------------------------------------------ the oracle step, as named tensors
def faulty_score(seq, memory, ptr, fault):
    if fault == "score_plus1":  # memory[:ptr + 1]: one row past the fill level
        if ptr < 10:
            return torch.zeros(seq.shape[0])
        sim = torch.clamp(ae.safe_normalize(ae.nan0(seq)) @ ae.safe_normalize(ae.nan0(memory[:ptr + 1])).t(), -1, 1)
        return torch.clamp(torch.min(1 - sim, dim=1).values, 0, 2) / 2.0
    return ae.memory_score(seq, memory, ptr)


def faulty_update(memory, ptr, f, fault):
    if fault == "wrap_early":  # the ring write wraps one row early
        for r in range(f.shape[0]):
            memory[(ptr + r) % (MEM - 1)] = ae.nan0(f[r])
        return (ptr + f.shape[0]) % (MEM - 1)
    return ae.update_memory(memory, ptr, f)


def _nhwc(t):
    return t.detach().double().permute(0, 2, 3, 1).numpy()


def record_view(rec, T, training=True):
    """The forward's intermediates in the device's layouts (vad.h, vad_ae_debug_buffer)."""
    v = {}
    for l, bn in enumerate(ae.ENC_BNS):
        v[f"ey{l}"] = np.stack([_nhwc(rec[(bn, t)]["y"]) for t in range(T)])
        for k in ("mean", "invstd"):
            v[f"est{l}.{k}"] = np.stack([rec[(bn, t)][k].double().numpy() for t in range(T)])
    for j, bn in enumerate(ae.DEC_BNS):
        v[f"dy{j}"] = _nhwc(rec[(bn, 0)]["y"])
        for k in ("mean", "invstd"):
            v[f"dst{j}.{k}"] = rec[(bn, 0)][k].double().numpy()
    v["u"] = rec["u"].detach().double().numpy()
    for k in ("gx", "gates", "cs"):
        v[k] = torch.stack(rec[k]).detach().double().numpy()
    if training:
        v["dG"] = torch.stack([p.grad for p in rec["pre"]]).double().numpy()
    return v


def record_pins(rec, T):
    """ae_leaky_pins' rule on an oracle record: the exact sign of y * scale + shift (tests/golden_util.py)."""
    def mask(e, p, bn):
        inv = e["invstd"].double()
        scale = p[f"{bn}.weight"].double() * inv
        shift = p[f"{bn}.bias"].double() - e["mean"].double() * scale
        c = (None, slice(None), None, None)
        return e["y"].detach().double() * scale[c] + shift[c] > 0
    p = rec["params"]
    return {"enc": [[mask(rec[(bn, t)], p, bn) for bn in ae.ENC_BNS] for t in range(T)],
            "dec": [rec["u"].detach() > 0] + [mask(rec[(bn, 0)], p, bn) for bn in ae.DEC_BNS]}


def oracle_step(c, dtype, pins=None, fault=None):
    """train_model's iteration (ae_oracle.ae_train_step) on case c with every tensor the comparison names; the raw
    record under "_rec"."""
    params, bufs = _cast(c.params, dtype), _cast(c.bufs, dtype)
    leaves = {n: t.requires_grad_(True) for n, t in _cast(params, dtype).items()}
    ctx = {"record": {}, "fault": fault}
    x = c.x.to(dtype)
    out = ae.ae_forward(leaves, bufs, x, True, pins=pins, ctx=ctx)
    ring = c.ring.to(dtype).clone()
    score = faulty_score(out["sequence_feature"].detach(), ring, c.ptr, fault)
    loss = ae.safe_mse(out["reconstructed"], x)
    loss.backward()
    v = record_view(ctx["record"], c.T)
    v["lat"] = out["frame_features"].detach().double().transpose(0, 1).numpy()
    v["seq"] = out["sequence_feature"].detach().double().numpy()
    for k in ("reconstructed", "sequence_feature", "frame_features"):
        v[f"out.{k}"] = out[k].detach().double().numpy()
    v["out.anomaly_score"] = score.double().numpy()
    v["loss"] = float(loss.detach())
    grads = {n: t.grad.detach().clone() for n, t in leaves.items()}
    for n, g in grads.items():
        v[f"grad.{n}"] = g.double().numpy().copy()  # (the clip below scales g in place)
    for n, t in bufs.items():
        v[f"run.{n}"] = t.double().numpy()
    ptr = faulty_update(ring, c.ptr, out["sequence_feature"].detach(), fault)
    v["mem.ring"], v["mem.ptr"] = ring.double().numpy(), ptr
    ae.clip_grad_norm(grads, 0.1)
    adam_update(params, grads, {}, LR, 1e-6)
    for n, t in params.items():
        v[f"param.{n}"] = t.double().numpy()
    ctx["record"]["params"] = c.params
    v["_rec"] = ctx["record"]
    return v


def adam_refs(c, grads):
    """The parameters after clip_grad_norm_(0.1) + Adam on the given gradients {name: array}, in float64 and in
    float32, as {"param.<name>": float64 array}: the optimizer is judged on the gradient it was given
    (test_optim_gpu's method; the gradients have their own comparison)."""
    out = []
    for dtype in (torch.float64, torch.float32):
        p = _cast(c.params, dtype)
        g = {n: torch.from_numpy(np.array(grads[n], np.float64)).to(dtype).reshape(t.shape) for n, t in p.items()}
        ae.clip_grad_norm(g, 0.1)
        adam_update(p, g, {}, LR, 1e-6)
        out.append({f"param.{n}": t.double().numpy() for n, t in p.items()})
    return out


@functools.lru_cache(maxsize=None)
def cpu_steps(name):
    """(float32 step, float64 step) of a case, both pinned to the float32 step's own LeakyReLU decisions; the
    float64 step's parameters are those of the float32 step's gradients (adam_refs)."""
    c = case_of(name)
    pins = record_pins(oracle_step(c, torch.float32)["_rec"], c.T)
    s32, s64 = oracle_step(c, torch.float32, pins), oracle_step(c, torch.float64, pins)
    s64.update(adam_refs(c, {n: s32[f"grad.{n}"] for n in c.params})[0])
    return s32, s64, pins


# ------------------------------------------------------------------------------------------ the comparison
def compare(got, ref, f32, label, quiet=False):
    """Every named tensor of a step (device, or an oracle step standing in for it) against the float64 step, with the
    float32 step as the yardstick of the derived bounds.  Returns the names that miss their bound."""
    bad, lines = [], []
    for name, r in ref.items():
        if name.startswith("_") or name not in got:
            continue
        g = got[name]
        cls = name.split(".")[0].rstrip("0123456789")
        if name == "mem.ptr":
            ok, msg = g == r, f"{g} vs {r}"
        elif name == "loss":
            ok, msg = abs(g - r) <= 1e-5 * abs(r), f"{g:.8g} vs {r:.8g}"
        elif cls in ("out", "mem"):
            err = np.abs(g - r) - 1e-4 * np.abs(r)
            ok, msg = bool((err <= 1e-5).all()), f"max |d| - rtol |ref| {float(err.max()):.3g} / 1e-5"
        elif cls == "grad" and name[5:] in PRE_BN_BIASES:
            wn = float(np.linalg.norm(ref[name[:-4] + "weight"]))
            ok, msg = float(np.abs(g).max()) <= 1e-5 * wn + 1e-9, f"pre-BN bias grad {float(np.abs(g).max()):.3g}"
        elif cls == "grad":
            d = _rel(g, r)
            ok, msg = d <= TOL, f"rel-L2 {d:.3g} / {TOL:g} (float32 oracle {_rel(f32[name], r):.3g})"
        elif cls == "param":
            d = float(np.abs(g - r).max())
            lim = 2 * float(np.abs(f32[name] - r).max()) + 2.0 ** -23 * float(np.abs(r).max())
            ok, msg = d <= lim, f"max |d| {d:.3g} / {lim:.3g}"
        else:
            assert cls in INTERMEDIATE + ("run",), name
            d, d32 = _rel(g, r), _rel(f32[name], r)
            lim = max(TOL, 2.0 * d32)
            ok, msg = d <= lim, f"rel-L2 {d:.3g} / {lim:.3g} (float32 oracle {d32:.3g})"
        lines.append(f"  {label} {name}: {msg}{'' if ok else '  <-- FAILS'}")
        if not ok:
            bad.append(name)
    if not quiet:
        print("\n".join(lines))
    return bad


# ------------------------------------------------------------------------------------------ CPU companions
@pytest.mark.parametrize("name", IDS)
def test_float32_oracle_stays_inside_every_bound(name):
    """The bounds are reachable: the float32 CPU oracle, pinned like the device, passes the whole comparison."""
    s32, s64, _ = cpu_steps(name)
    assert compare(s32, s64, s32, f"{name}/float32") == []
    worst = {}
    for k in s64:
        cls = k.split(".")[0].rstrip("0123456789")
        if cls in INTERMEDIATE + ("run", "grad") and k[5:] not in PRE_BN_BIASES:
            worst[cls] = max(worst.get(cls, 0.0), _rel(s32[k], s64[k]))
    print(name, "float32 oracle vs float64, worst rel-L2 per class:", " ".join(f"{k}={v:.2e}" for k, v in worst.items()))


# fault -> (the cases where it acts, a tensor whose comparison must catch it there)
FAULTS = {
    "drop_tail": (("b5t3", "est2.mean"), ("b5t3", "dst0.mean"), ("b17t1", "est3.mean"), ("b17t1", "est3.invstd")),
    "g17_skip": (("b2t17", "est0.mean"), ("b2t17", "run.encoder.10.running_mean"), ("b2t33", "est3.invstd")),
    "g17_stale": (("b2t17", "est0.mean"), ("b2t17", "run.encoder.1.running_var"), ("b2t33", "est2.mean")),
    "biased_var": (("b1t1", "run.encoder.10.running_var"), ("b1t2", "run.encoder.10.running_var"),
                   ("b5t3", "run.encoder.10.running_var"), ("b1t2", "run.decoder.7.running_var")),
    "dec_once": (("b1t2", "run.decoder.4.running_mean"), ("b2t17", "run.decoder.10.running_var"),
                 ("b5t3", "run.decoder.7.running_mean")),
    "wrap_early": (("b5t3", "mem.ring"), ("b5t3", "mem.ptr"), ("b17t1", "mem.ring"), ("b2t17", "mem.ptr")),
    "score_plus1": (("b1t2", "out.anomaly_score"), ("b17t1", "out.anomaly_score"), ("b2t33", "out.anomaly_score")),
}


def _no_params(step):
    """(no fault touches the optimizer, and its reference belongs to the float32 step's gradients: cpu_steps)"""
    return {k: v for k, v in step.items() if not k.startswith("param.")}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_injected_faults_are_caught(fault):
    """Each fault, restated on the oracle's side in float64, fails the comparison that should catch it; where it does
    not act (no partial tile, T <= 16, ...) the faulty step passes, so the catch is the fault's and not noise."""
    for name in sorted({n for n, _ in FAULTS[fault]}):
        s32, s64, pins = cpu_steps(name)
        bad = compare(_no_params(oracle_step(case_of(name), torch.float64, pins, fault)), s64, s32, f"{name}/{fault}",
                      quiet=True)
        print(name, fault, "fails:", " ".join(bad[:12]))
        for n, tensor in FAULTS[fault]:
            if n == name:
                assert tensor in bad, (fault, name, tensor)
    idle = {"drop_tail": "b2t17", "g17_skip": "b5t3", "g17_stale": "b5t3", "dec_once": "b17t1", "wrap_early": "b2t33",
            "score_plus1": "b1t1", "biased_var": None}[fault]
    if idle:
        s32, s64, pins = cpu_steps(idle)
        assert compare(_no_params(oracle_step(case_of(idle), torch.float64, pins, fault)), s64, s32, idle,
                       quiet=True) == []


def test_table_reaches_its_regimes():
    """Plain arithmetic of the grouped BN (256-row tiles, 16 groups per pass) and the implicit GEMMs (64-row tiles,
    split K under 512 tiles): the cases reach what REGIMES claims."""
    cdiv = lambda a, b: -(-a // b)  # noqa: E731

    def bn(B, rows_per_clip):
        mg = B * rows_per_clip
        return mg, cdiv(mg, R_TILE), mg % R_TILE

    def gemm(M, N, K):
        tiles = cdiv(M, 64) * cdiv(N, 64)
        return tiles, (min(cdiv(1024, tiles), K // 64) if tiles < 512 else 1)

    by = {r["name"]: r for r in REGIMES}
    assert bn(1, 16) == (16, 1, 16)                       # b1: enc layer 3, 16 values per channel
    assert 16 / 15 == pytest.approx(1.0667, abs=1e-4)     # ... and its unbiased-variance factor
    assert bn(5, 64) == (320, 2, 64)                      # b5t3: enc layer 2 and dec BN 0, P = 2 with a 64-row tail
    assert bn(17, 16) == (272, 2, 16)                     # b17t1: enc layer 3, a 16-row tail tile
    for name in ("b1t1", "b1t2"):                         # every decoder GEMM of B = 1: a partial 64-row tile, split K
        B = by[name]["B"]
        for ci, co, hw in DEC:
            M = B * (hw // 2) ** 2                        # rows per parity class of the transposed conv
            assert 16 <= M <= 1024 and (M < 64 or M % 64 == 0)
            assert gemm(M, co, 4 * ci)[1] > 1
        assert B * 16 == 16 and gemm(16, 128, 16 * 128)[1] > 1   # enc layer 3: M = 16 rows
    passes = {n: cdiv(by[n]["T"], 16) for n in by}
    assert passes == dict(b1t1=1, b1t2=1, b5t3=1, b17t1=1, b2t17=2, b2t33=3)
    assert by["b2t17"]["T"] % 16 == 1 and by["b2t33"]["T"] % 16 == 1   # the last pass holds one group, 15 idle lanes
    assert [by[n]["T"] for n in ("b1t1", "b17t1")] == [1, 1]           # G = 1, repeat = 1 in training
    ring = {n: (by[n]["ptr"], by[n]["ptr"] + by[n]["B"]) for n in by}
    assert ring["b1t1"][0] == 9 and ring["b1t2"][0] == 10               # the fill boundary
    assert ring["b5t3"][1] == MEM                                       # exact fill
    assert ring["b17t1"][1] > MEM and ring["b2t17"] == (499, 501)       # wraps in mid-batch
    assert ring["b2t33"][0] == R_TILE + 1                               # the score's row loop: a second stride of 1


# ------------------------------------------------------------------------------------------ the device
def device_view(plan, B, T, training=True):
    from tests.golden_util import read_ae_debug
    rd = lambda n, i=0: read_ae_debug(plan, n, i).astype(np.float64)  # noqa: E731
    v = {}
    for l, (_, C, hw) in enumerate(ENC):
        v[f"ey{l}"] = rd("ey", l).reshape(T, B, hw, hw, C)
        st = rd("est", l).reshape(T, 8, C)
        v[f"est{l}.mean"], v[f"est{l}.invstd"] = st[:, 0], st[:, 1]
    for j, (_, C, hw) in enumerate(DEC):
        v[f"dy{j}"] = rd("dy", j).reshape(B, hw, hw, C)
        st = rd("dst", j).reshape(8, C)
        v[f"dst{j}.mean"], v[f"dst{j}.invstd"] = st[0], st[1]
    v["u"] = rd("u").reshape(B, 2048)
    for k, w in (("lat", 64), ("gx", 256), ("gates", 256), ("cs", 64)) + ((("dG", 256),) if training else ()):
        v[k] = rd(k).reshape(T, B, w)
    v["seq"] = rd("seq").reshape(B, 64)
    return v


def _d(t):
    return t.detach().cpu().double().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("direct", [1, 0], ids=["direct", "im2col"])
@pytest.mark.parametrize("name", IDS)
def test_train_step_matches_float64_layer_by_layer(name, direct):
    from vad_amd import _native as nat
    from vad_amd.ae import AeTrainer
    from tests.golden_util import ae_leaky_pins
    c = case_of(name)
    B, T = c.B, c.T
    nat.check(nat.lib().vad_set_tuning(b"ae_direct", direct))
    try:
        fwd = c.model().cuda().train()
        with torch.no_grad():
            out = fwd(c.x.cuda())
        model = c.model().cuda()
        tr = AeTrainer(model, lr=LR)
        l = tr.step(c.x.cuda()).cpu().numpy()
        assert int(l[3]) == 2
        e = model.engine()
        plan = e.plans[(B, T)]
        got = device_view(plan, B, T)
        pins = ae_leaky_pins(plan, B, T)
        for k in ("reconstructed", "sequence_feature", "frame_features", "anomaly_score"):
            got[f"out.{k}"] = _d(out[k])
        got["loss"] = float(l[0])
        for n, g in e.grad_dict().items():
            got[f"grad.{n}"] = _d(g).reshape(c.params[n].shape)
        sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    finally:
        nat.check(nat.lib().vad_set_tuning(b"ae_direct", 1))
    for n, t in sd.items():
        if "running" in n:
            got[f"run.{n}"] = t.double().numpy()
        elif "num_batches" in n:
            assert int(t) == T, n  # one update per frame index (encoder) / per decoder call, exactly
        elif n in c.params:
            got[f"param.{n}"] = t.double().numpy()
    got["mem.ring"], got["mem.ptr"] = sd["normal_memory"].double().numpy(), int(sd["memory_ptr"][0])
    # the ring is a copy: bit-equal to the oracle's update with the device's own sequence features
    ring = c.ring.clone()
    ptr = ae.update_memory(ring, c.ptr, torch.from_numpy(got["seq"].astype(np.float32)))
    assert got["mem.ptr"] == ptr
    assert torch.equal(sd["normal_memory"], ring)
    s64 = oracle_step(c, torch.float64, pins)
    s32 = oracle_step(c, torch.float32, pins)
    for s, p in zip((s64, s32), adam_refs(c, {n: got[f"grad.{n}"] for n in c.params})):
        s.update(p)
    bad = compare(got, s64, s32, f"{name}/{'direct' if direct else 'im2col'}")
    assert not bad, bad


def eval_bufs(c):
    """Non-default running statistics: means of the size of the activations' spread, variances in [0.5, 2]."""
    gen = torch.Generator().manual_seed(c.seed + 1000)
    out = {}
    for k, v in c.bufs.items():
        if k.endswith("running_mean"):
            out[k] = 0.3 * torch.randn(v.shape, generator=gen)
        else:
            out[k] = 0.5 + 1.5 * torch.rand(v.shape, generator=gen)
    return out


def oracle_eval(c, bufs, dtype, weights, pins=None):
    leaves = {n: t.requires_grad_(True) for n, t in _cast(c.params, dtype).items()}
    ctx = {"record": {}}
    out = ae.ae_forward(leaves, _cast(bufs, dtype), c.x.to(dtype), False, c.ring.to(dtype), c.ptr, pins=pins, ctx=ctx)
    sum((out[k] * w.to(dtype)).sum() for k, w in weights.items()).backward()
    v = record_view(ctx["record"], c.T, training=False)
    v["lat"] = out["frame_features"].detach().double().transpose(0, 1).numpy()
    v["seq"] = out["sequence_feature"].detach().double().numpy()
    for k in out:
        v[f"out.{k}"] = out[k].detach().double().numpy()
    for n, t in leaves.items():
        v[f"evalgrad.{n}"] = t.grad.double().numpy()
    ctx["record"]["params"] = c.params
    v["_rec"] = ctx["record"]
    return v


def eval_weights(c):
    gen = torch.Generator().manual_seed(c.seed + 2000)
    return {"reconstructed": torch.randn(c.B, c.T, 1, 64, 64, generator=gen),
            "sequence_feature": torch.randn(c.B, 64, generator=gen),
            "frame_features": torch.randn(c.B, c.T, 64, generator=gen)}


def compare_eval(got, ref, f32, label):
    """compare() for the eval pass: in eval mode BN is an affine map, so the pre-BN biases have real gradients and
    every gradient tensor takes the pinned bound."""
    bad = compare({k: v for k, v in got.items() if not k.startswith("evalgrad")}, ref, f32, label)
    for k, r in ref.items():
        if k.startswith("evalgrad."):
            d = _rel(got[k], r)
            print(f"  {label} {k}: rel-L2 {d:.3g} / {TOL:g} (float32 oracle {_rel(f32[k], r):.3g})")
            if not d <= TOL:
                bad.append(k)
    return bad


@pytest.mark.parametrize("name", IDS)
def test_float32_oracle_stays_inside_every_eval_bound(name):
    c = case_of(name)
    bufs, w = eval_bufs(c), eval_weights(c)
    pins = record_pins(oracle_eval(c, bufs, torch.float32, w)["_rec"], c.T)
    s32, s64 = oracle_eval(c, bufs, torch.float32, w, pins), oracle_eval(c, bufs, torch.float64, w, pins)
    assert compare_eval(s32, s64, s32, f"{name}/eval/float32") == []


@pytest.mark.gpu
@pytest.mark.parametrize("direct", [1, 0], ids=["direct", "im2col"])
@pytest.mark.parametrize("name", IDS)
def test_eval_forward_and_autograd_match_float64(name, direct):
    """Eval mode with non-default running stats: the forward, and the module's autograd through it (the eval branch of
    gbn_bwd_finalize_kernel: no batch-mean terms), against the oracle's autograd; nothing in the state moves."""
    from vad_amd import _native as nat
    from tests.golden_util import ae_leaky_pins
    c = case_of(name)
    B, T = c.B, c.T
    bufs, w = eval_bufs(c), eval_weights(c)
    nat.check(nat.lib().vad_set_tuning(b"ae_direct", direct))
    try:
        model = c.model(bufs).cuda().eval()
        before = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        out = model(c.x.cuda())
        sum((out[k] * w[k].cuda()).sum() for k in w).backward()
        plan = model.engine().plans[(B, T)]
        got = device_view(plan, B, T, training=False)
        pins = ae_leaky_pins(plan, B, T)
        for k in ("reconstructed", "sequence_feature", "frame_features", "anomaly_score"):
            got[f"out.{k}"] = _d(out[k])
        for n, p in model.named_parameters():
            got[f"evalgrad.{n}"] = _d(p.grad)
        after = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    finally:
        nat.check(nat.lib().vad_set_tuning(b"ae_direct", 1))
    for k, v in before.items():
        assert torch.equal(v, after[k]), k
    s64, s32 = oracle_eval(c, bufs, torch.float64, w, pins), oracle_eval(c, bufs, torch.float32, w, pins)
    bad = compare_eval(got, s64, s32, f"{name}/eval/{'direct' if direct else 'im2col'}")
    assert not bad, bad


# ------------------------------------------------------------------------------------------ the memory kernels alone
def _ring_model():
    return make_ae_model(dict(seed=80, mem=None)).cuda().eval()


@pytest.mark.gpu
def test_memory_update_is_exact_at_every_wrap_position():
    model = _ring_model()
    gen = torch.Generator().manual_seed(81)
    for ptr, n in ((0, 1), (483, 17), (490, 17), (499, 1), (499, 2), (250, 500)):
        ring = torch.randn(MEM, 64, generator=gen)
        f = torch.randn(n, 64, generator=gen)
        f[0, 3] = float("nan")  # stored as 0 (check_and_fix_nan, cad1:204)
        f[n - 1, 63] = float("nan")
        with torch.no_grad():
            model.normal_memory.copy_(ring)
            model.memory_ptr.fill_(ptr)
        model.update_memory(f.cuda())
        want = ae.update_memory(ring, ptr, f)
        assert int(model.memory_ptr[0]) == want, (ptr, n)
        assert torch.equal(model.normal_memory.cpu(), ring), (ptr, n)
        assert not bool(torch.isnan(model.normal_memory).any())


def _scores(model, ring, fill, s):
    with torch.no_grad():
        model.normal_memory.copy_(ring)
        model.memory_ptr.fill_(fill)
    return model.compute_anomaly_score(s.cuda()).cpu()


def _exact_feature():
    """16 entries of +-0.75: norm 3 and cosines of +-1 exactly, in float32 and in any summation order."""
    f = torch.zeros(64)
    f[::4] = 0.75
    f[4::8] = -0.75
    return f


@pytest.mark.gpu
@pytest.mark.parametrize("fill", [9, 10, 255, 256, 257, 499])
def test_memory_score_at_fill_and_stride_boundaries(fill):
    """The nearest row sits last, at fill - 1 (a short loop misses it); the rows from fill on hold the features
    themselves (a long loop finds them and scores 0)."""
    model = _ring_model()
    gen = torch.Generator().manual_seed(82 + fill)
    for n in (1, 5):
        s = torch.randn(n, 64, generator=gen)
        ring = torch.randn(MEM, 64, generator=gen)
        ring[fill - 1] = s[n - 1] + 0.05 * torch.randn(64, generator=gen)
        ring[fill] = s[n - 1]
        ring[fill + 1:] = s[0]
        ring[0] = 0.0  # a zero-norm row: the 1e-8 clamp, cosine 0
        got = _scores(model, ring, fill, s)
        want = ae.memory_score(s.double(), ring.double(), fill)
        if fill < 10:
            assert torch.equal(got, torch.zeros(n))
            continue
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-5, atol=1e-6)
        assert 1e-4 < float(want[n - 1]) < 0.01  # the last row is the nearest, and is not the feature itself


@pytest.mark.gpu
def test_memory_score_edges_zero_clamp_and_nan():
    model = _ring_model()
    gen = torch.Generator().manual_seed(90)
    fill = 40
    base = torch.randn(MEM, 64, generator=gen)
    f = _exact_feature()
    # an all-zero sequence feature: every cosine 0, score 1/2 exactly; beside it the exact feature and a random one
    s = torch.stack([torch.zeros(64), f, torch.randn(64, generator=gen)])
    ring = base.clone()
    ring[7] = 0.0
    got = _scores(model, ring, fill, s)
    want = ae.memory_score(s.double(), ring.double(), fill)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-5, atol=1e-6)
    assert float(got[0]) == 0.5
    # a ring row equal to the feature: exactly 0, never negative (cos clamped at 1)
    ring = base.clone()
    ring[fill - 1] = f
    got = _scores(model, ring, fill, s)
    assert float(got[1]) == 0.0 and bool((got >= 0).all())
    ring[fill - 1] = 3.0 * s[2]  # the same direction at another norm: cos rounds to either side of 1
    got = _scores(model, ring, fill, s)
    assert 0.0 <= float(got[2]) <= 1e-6
    # a ring that holds only the negated feature: cos -1, score 1
    ring = (-f).repeat(MEM, 1)
    assert float(_scores(model, ring, fill, s)[1]) == 1.0
    # NaN in the feature: that element counts as 0 (check_and_fix_nan, cad1:266)
    sn = s.clone()
    sn[2, 5] = float("nan")
    ring = base.clone()
    got = _scores(model, ring, fill, sn)
    want = ae.memory_score(sn.double(), ring.double(), fill)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-5, atol=1e-6)


@pytest.mark.gpu
def test_memory_score_fixes_nan_in_the_nearest_row():
    """The reference NaN-fixes the populated ring before normalising it (cad1:272): a row that is the nearest one but
    for one NaN element (a ring loaded from a state_dict) stays the nearest, with that element 0."""
    model = _ring_model()
    gen = torch.Generator().manual_seed(91)
    fill = 300
    s = torch.randn(5, 64, generator=gen)
    ring = torch.randn(MEM, 64, generator=gen)
    ring[fill - 1] = s[3] + 0.05 * torch.randn(64, generator=gen)
    ring[fill - 1, 11] = float("nan")
    ring[2] = s[0]
    ring[2, 0] = float("nan")
    got = _scores(model, ring, fill, s)
    want = ae.memory_score(s.double(), ring.double(), fill)
    print("NaN-row scores: device", got.numpy(), "float64", want.numpy())
    assert float(want[3]) < 0.05 and float(want[0]) < 0.05
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-5, atol=1e-6)
