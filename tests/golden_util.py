"""Helpers shared by the parity tests: golden fixture loading and reference-identical model construction."""
import contextlib
import glob
import os

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# the reference's shipped a2 checkpoint (best_improved_model.pth, model_state_dict) exported as a safe .npz
A2_CKPT = "a2_best_improved_model.npz"


def load(name):
    return dict(np.load(os.path.join(GOLDEN_DIR, name), allow_pickle=False))


@contextlib.contextmanager
def recording_threads():
    """The torch CPU thread count the golden vectors were recorded at (8, make_golden.py): torch splits CPU sums by
    its thread count, so comparisons at rounding level hold only on that partition, whatever the host's CPU count or
    OMP_NUM_THREADS."""
    n = torch.get_num_threads()
    torch.set_num_threads(8)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def init_checksums(t):
    """(sum, sum of squares) of a tensor in float64, as make_golden.py recorded them (init_sum / init_sq)."""
    with recording_threads():
        return np.float64(t.double().sum()), np.float64((t.double() ** 2).sum())


def cad_cases():
    from tests.golden.cases import CAD_CASES
    return CAD_CASES


def make_cad_model(case):
    """Our drop-in module under the case seed (identical init to the reference), with the forced-detector edit."""
    from vad_amd.cad import CausalAnomalyDetector
    from tests.golden.cases import force_detector
    torch.manual_seed(case["seed"])
    m = CausalAnomalyDetector(num_factors=6, reid_dim=64)
    if case["forced"]:
        force_detector(m.state_dict(), case["forced"])
    return m


EPS_REGIME_VAR = 1e-7  # running_var of the two channels per layer whose invstd is decided by eps = 1e-5
CALIBRATION_FRAMES = 8


def calibrated_bn_state(sd, case, seed):
    """A copy of the cad state dict sd with the nine backbone BatchNorm layers in a trained-like state, on the CPU and
    deterministic from seed (one torch.Generator, drawn layer by layer in oracle.cad_oracle.BN_LAYERS order: sign,
    gamma, beta, mean noise, variance factor, eps-regime channels).  case: its "H", "W" size the calibration clip.
      * gamma = s * U[0.5, 1.5], s = -1 on about a quarter of the channels (bn1 too: the frozen stem's min arm);
        beta ~ N(0, 0.3);
      * running_mean / running_var: the per-channel batch mean and unbiased variance of each layer's pre-BN map in one
        float64 train-mode oracle forward of CALIBRATION_FRAMES synthetic frames of the case's size under the gamma and
        beta above (every layer sees a network normalised below it), the mean times 1 + 0.1 n, n ~ N(0, 1), the
        variance times U[0.5, 2];
      * two channels per layer in the eps regime: running_var = EPS_REGIME_VAR, and gamma scaled by
        sqrt((EPS_REGIME_VAR + eps) / (var + eps)) so that the channel's output is what it was with var;
      * num_batches_tracked = 1000 + the layer's index.
    Everything else (detector, heads: force_detector is applied before, as make_cad_model does) is untouched."""
    from oracle import cad_oracle as co
    g = torch.Generator().manual_seed(seed)
    out = {k: v.detach().clone() for k, v in sd.items()}
    draws = []
    for bn, C in zip(co.BN_LAYERS, co.BN_CHANNELS):
        sign = torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
        out[bn + ".weight"] = sign * (0.5 + torch.rand(C, generator=g))
        out[bn + ".bias"] = 0.3 * torch.randn(C, generator=g)
        draws.append((torch.randn(C, generator=g, dtype=torch.float64),
                      0.5 + 1.5 * torch.rand(C, generator=g, dtype=torch.float64),
                      torch.randperm(C, generator=g)[:2]))
    p = {k: v.double() for k, v in out.items() if "running" not in k and "num_batches" not in k}
    bufs = {k: v.double().clone() for k, v in out.items() if "running" in k}
    x = co.synth_clips(seed, 0, 0, 1, CALIBRATION_FRAMES, case["H"], case["W"]).double()
    rec = {}
    with torch.no_grad():
        co.backbone_forward(p, bufs, x, training=True, record=rec)
    for i, (bn, (n, u, epsc)) in enumerate(zip(co.BN_LAYERS, draws)):
        y = rec["y_stem"] if i == 0 else rec[f"y{i - 1}"].detach()
        mean = y.mean((0, 2, 3)) * (1 + 0.1 * n)
        var = y.var((0, 2, 3), unbiased=True) * u
        gamma = out[bn + ".weight"].double()
        gamma[epsc] *= torch.sqrt((EPS_REGIME_VAR + 1e-5) / (var[epsc] + 1e-5))
        var[epsc] = EPS_REGIME_VAR
        out[bn + ".weight"] = gamma.float()
        out[bn + ".running_mean"] = mean.float()
        out[bn + ".running_var"] = var.float()
        out[bn + ".num_batches_tracked"] = torch.tensor(1000 + i, dtype=torch.int64)
    return out


def ae_memory_init(case):
    """(normal_memory (500, 64), memory_ptr) of a cad1 AE case before training."""
    mem = torch.zeros(500, 64)
    if case["mem"] is None:
        return mem, 0
    rows, ptr = case["mem"]
    mem[:rows] = torch.from_numpy(np.random.default_rng(case["seed"]).standard_normal((rows, 64)).astype(np.float32))
    return mem, ptr


def ae_case_data(case):
    """(train, val, test) lists of (clips (B, T, 1, 64, 64), int64 labels) of a cad1 AE case."""
    from oracle import ae_oracle as ae
    B, T, seed = case["B"], case["T"], case["seed"]
    lab = lambda v: torch.tensor(v, dtype=torch.int64)  # noqa: E731
    train = [(ae.synth_clips(seed, k, k * B, B, T), lab(y)) for k, y in enumerate(case["labels"])]
    val = [(ae.synth_clips(seed, 100, 0, len(case["val_labels"]), T), lab(case["val_labels"]))]
    test = [(ae.synth_clips(seed, 200, 0, len(case["test_labels"]), T), lab(case["test_labels"]))]
    return train, val, test


def golden_names():
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN_DIR, "*.npz")))


# ---------------------------------------------------------------- mask-pinned oracle gradients (GPU tests)
def read_ae_debug(plan, name, idx=0):
    """Copy a cad1 plan's debug buffer (vad_ae_debug_buffer) to the host (float32)."""
    import ctypes
    from vad_amd import _native as nat
    p, k = ctypes.c_void_p(), ctypes.c_int64()
    nat.check(nat.lib().vad_ae_debug_buffer(plan.h, name.encode(), idx, ctypes.byref(p), ctypes.byref(k)))
    out = np.empty(k.value, np.float32)
    nat.check(nat.lib().vad_debug_d2h(out.ctypes.data, p.value, out.nbytes))
    return out


def ae_leaky_pins(plan, B, T):
    """The LeakyReLU decisions of the device's last cad1 forward, in the oracle's layout (ae_oracle.ae_forward pins):
    the sign of y * scale + shift computed exactly in float64 from the device's raw conv outputs and BN state (the
    device's fp32 fma decision), and of the decoder Linear's output."""
    from oracle import ae_oracle as ae
    enc_hw = (32, 16, 8, 4)
    enc = [[None] * 4 for _ in range(T)]
    for l in range(4):
        C, hw = (32, 64, 128, 128)[l], enc_hw[l]
        y = read_ae_debug(plan, "ey", l).astype(np.float64).reshape(T, B, hw, hw, C)
        st = read_ae_debug(plan, "est", l).astype(np.float64).reshape(T, 8, C)
        z = y * st[:, None, None, None, 2, :] + st[:, None, None, None, 3, :]
        m = torch.from_numpy(np.ascontiguousarray((z > 0).transpose(0, 1, 4, 2, 3)))
        for t in range(T):
            enc[t][l] = m[t]
    dec = [torch.from_numpy(read_ae_debug(plan, "u").reshape(B, 2048) > 0)]
    for j in range(3):
        C, hw = (128, 64, 32)[j], (8, 16, 32)[j]
        y = read_ae_debug(plan, "dy", j).astype(np.float64).reshape(B, hw, hw, C)
        st = read_ae_debug(plan, "dst", j).astype(np.float64).reshape(8, C)
        dec.append(torch.from_numpy(np.ascontiguousarray((y * st[2] + st[3] > 0).transpose(0, 3, 1, 2))))
    assert len(ae.ENC_CONVS) == 4
    return {"enc": enc, "dec": dec}
def read_debug(plan, name, idx=0, n=None, dtype=np.float32):
    """Copy a plan's debug buffer (vad_cad_debug_buffer) to the host."""
    import ctypes
    from vad_amd import _native as nat
    p, k = ctypes.c_void_p(), ctypes.c_int64()
    nat.check(nat.lib().vad_cad_debug_buffer(plan.h, name.encode(), idx, ctypes.byref(p), ctypes.byref(k)))
    n = k.value if n is None else n
    out = np.empty(n, dtype)
    nat.check(nat.lib().vad_debug_d2h(out.ctypes.data, p.value, out.nbytes))
    return out


def read_act(plan, name, idx=0, n=None):
    """A backbone activation buffer as float64, whatever its storage (fp32, or bf16 when the plan ran act_bf16):
    pool, y, and the backward's dA / dY (n: their element count -- dA is one buffer of the largest map's size)."""
    if int(read_debug_len(plan, "act_bf16")) == 1 and name in ("y", "pool", "dA", "dY"):
        u = read_debug(plan, name, idx, n=n, dtype=np.uint16)
        return (u.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return read_debug(plan, name, idx, n=n).astype(np.float64)


def read_debug_len(plan, name, idx=0):
    import ctypes
    from vad_amd import _native as nat
    p, k = ctypes.c_void_p(), ctypes.c_int64()
    nat.check(nat.lib().vad_cad_debug_buffer(plan.h, name.encode(), idx, ctypes.byref(p), ctypes.byref(k)))
    return k.value


def hip_relu_masks(eng, NF):
    """The ReLU decisions the HIP forward took after the eight 3x3-conv BatchNorms: relu(fma(y, scale, shift)) is
    taken iff the exact value y*scale + shift > 0.  y*scale is exact in float64 (24-bit x 24-bit mantissas) and the
    float64 add keeps the sign, so the comparison reproduces the device's fp32 fma decision bit for bit (bf16-stored
    activations are widened exactly first).
    Returns 8 bool tensors (NF, C, OH, OW) for oracle.cad_oracle.backbone_forward(relu_masks=...)."""
    pl = eng._last[0]
    masks = []
    for l in range(8):
        st = read_debug(pl, "stats", l + 1)
        C = st.size // 7  # BN stats layout [7C] (csrc/common.h BN_STATS_PER_C)
        y = read_act(pl, "y", l).reshape(NF, -1, C)
        z = y * st[2 * C:3 * C].astype(np.float64) + st[3 * C:4 * C].astype(np.float64)
        masks.append(torch.from_numpy(z > 0).permute(0, 2, 1))  # (NF, C, OH*OW); pinned_oracle_grads reshapes
    return masks


def hip_stem_pins(eng, NF, H, W):
    """The training stem's decisions in the HIP forward (option stem_grad: conv1's output y1 stored): bn1's ReLU
    mask (exact sign of y1*scale + shift, as hip_relu_masks) and the MaxPool2d(3, 2, 1) window maxima under torch's
    first-max rule (strict >, row-major window scan) over z = relu(fma(y1, scale, shift)) rounded to fp32 as the
    device computes it (backbone.hip maxpool_bwd_kernel).  Returns (mask (NF, 32, H1, W1) bool, idx (NF, 32, HP, WP)
    int64 flat indices into each H1 x W1 plane) for backbone_forward(stem_pins=...)."""
    pl = eng._last[0]
    H1, W1 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    HP, WP = (H1 - 1) // 2 + 1, (W1 - 1) // 2 + 1
    st = read_debug(pl, "stats", 0).astype(np.float64)
    y1 = read_debug(pl, "y1").astype(np.float64).reshape(NF, H1, W1, 32)
    zz = y1 * st[64:96] + st[96:128]
    mask = zz > 0
    idx = first_max_pool_idx(np.maximum(zz.astype(np.float32), np.float32(0)))
    return (torch.from_numpy(mask).permute(0, 3, 1, 2).contiguous(),
            torch.from_numpy(idx).permute(0, 3, 1, 2).contiguous())


def first_max_pool_idx(z):
    """MaxPool2d(3, 2, 1) window maxima of an NHWC array as flat indices into each H x W plane, torch's rule: scan
    the window row-major, take a value when it is strictly greater than the best so far (padding never wins).
    Returns (N, OH, OW, C) int64."""
    N, H, W, C = z.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    zp = np.full((N, H + 2, W + 2, C), -np.inf, z.dtype)
    zp[:, 1:-1, 1:-1] = z
    best = np.full((N, OH, OW, C), -np.inf, z.dtype)
    idx = np.zeros((N, OH, OW, C), np.int64)
    oy = np.arange(OH)[:, None] * 2
    ox = np.arange(OW)[None, :] * 2
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            v = zp[:, oy + 1 + dy, ox + 1 + dx]
            better = v > best
            best = np.where(better, v, best)
            idx = np.where(better, ((oy + dy) * W + (ox + dx))[None, :, :, None], idx)
    return idx


def reshape_masks(masks, x):
    """hip_relu_masks output (NF, C, OH*OW) -> the (NF, C, OH, OW) tensors backbone_forward takes."""
    from oracle import cad_oracle as co
    shapes = []
    NF = x.shape[0] * x.shape[1]
    h, w = (x.shape[3] - 1) // 2 + 1, (x.shape[4] - 1) // 2 + 1
    h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    for _, _, s in co.BACKBONE_CONVS:
        h, w = (h - 1) // s + 1, (w - 1) // s + 1
        shapes.append((h, w))
    return [m.reshape(NF, m.shape[1], hh, ww) for m, (hh, ww) in zip(masks, shapes)]


def pinned_oracle_grads(state_dict, x, labels, draws, masks, sync_group=None, bf16=False, dtype=torch.float64,
                        head_masks=None, det_masks=None, fault=None, reverse_channels=False, stem_pins=None):
    """float64 oracle forward/backward of one train step with the ReLU decisions of another forward (masks from
    hip_relu_masks): the exact gradient of that forward's piecewise-linear branch, free of kink flips.  Returns
    (grads {name: float64 tensor or None}, losses {name: float64}, the oracle's result dict incl. "bufs" and
    "record" -- the float64 BatchNorm outputs "z{l}" in front of each pinned ReLU, for check_mask_flips).
    bf16: the backbone as the device computes it in bf16 mode (cad_oracle.backbone_forward_bf16; "reversed": its convs
    sum the input channels in reverse order).  dtype: the oracle's arithmetic (float64; float32 gives further,
    independent restatements at fp32 accumulation).  head_masks: the direct classifier's ReLU decisions too
    (cad_oracle.direct_forward's masks; its pre-activations land in record["dir_z{i}"]); det_masks: the detector
    MLP's likewise (record["det_z{i}"]); fault: backbone_forward_bf16's ragged-edge faults or, on the exact path,
    backbone_forward's (tests of the bounds); reverse_channels: the exact path's convs sum their input channels in reverse
    order; stem_pins: hip_stem_pins' decisions of a training stem -- conv1 and bn1 then train too."""
    from oracle import cad_oracle as co
    params = {k: v.detach().to(dtype).clone() for k, v in state_dict.items()
              if "running" not in k and "num_batches" not in k}
    bufs = {k: v.detach().to(dtype).clone() for k, v in state_dict.items() if "running" in k}
    xd = x.to(dtype)
    rm = reshape_masks(masks, xd)
    record = {}
    kw = dict(bf16=bf16) if bf16 else {}
    if head_masks is not None:
        kw["head_masks"] = head_masks
    if det_masks is not None:
        kw["det_masks"] = det_masks
    if fault is not None:
        kw["fault"] = fault
    if reverse_channels:
        kw["reverse_channels"] = True
    if stem_pins is not None:
        kw.update(stem_pins=stem_pins, train_stem=True)
    res = co.cad_train_step(params, bufs, {}, xd, labels, draws, relu_masks=rm, sync_group=sync_group,
                            record=record, **kw)
    res["bufs"] = bufs  # running stats after the step's forward
    res["record"] = record
    return res["grads"], res["losses"], res


def check_mask_flips(masks, record, x, ulps=64, unit=2.0 ** -24, accum=True):
    """The mask-pinned method takes the device's ReLU decisions; this bounds them: a decision may differ from the sign
    of the float64 oracle's own BatchNorm output z (the pinned oracle forward, record["z{l}"], i.e. the same branch
    taken in the layers below) only where |z| <= ulps units of the accumulation magnitude of that layer's conv,
    unit * sqrt(K) * RMS_c(z) per channel (K = 9 Ci: a K-term fp32 sum carries ~sqrt(K) roundings of the terms'
    scale; accum=False: unit * RMS_c(z), for bf16 storage whose one rounding of y dominates).  Returns per layer
    (flips, largest |z| at a flip / its bound); raises if a flip lies outside the bound."""
    from oracle import cad_oracle as co
    rm = reshape_masks(masks, x.double())
    out = []
    cin = [32, 32, 32, 64, 64, 128, 128, 256]
    for l, m in enumerate(rm):
        z = record[f"z{l}"]
        rms = z.pow(2).mean(dim=(0, 2, 3)).sqrt()[None, :, None, None]
        bound = ulps * unit * ((9 * cin[l]) ** 0.5 if accum else 1.0) * rms
        flips = (z > 0) != m.to(torch.bool)
        n = int(flips.sum())
        worst = float((z.abs() / bound)[flips].max()) if n else 0.0
        bad = flips & (z.abs() > bound)
        assert not bool(bad.any()), (f"layer {l}: {int(bad.sum())} of {n} ReLU decisions differ from the float64 "
                                     f"forward beyond {ulps} ulp of the accumulation scale (worst |z|/bound {worst:.3g})")
        out.append((n, worst))
    return out


def rel_l2(a, b):
    a = np.asarray(a, np.float64).reshape(-1)
    b = np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


# ---------------------------------------------------------------- bf16 mode against its restatements
# The spread a correct bf16 implementation may show against the float64 restatement, in units of the float32
# restatements' own distance to it (tests/test_cad_gpu.py has the derivation).
BF16_SPREAD = 2.0


def bf16_step_references(sd, x, y, draws, masks, hm, det_masks=None):
    """The four pinned oracle steps a bf16 step is judged by, each pinned_oracle_grads' (grads, losses, result):
    "ref" the float64 restatement of the device's bf16 rounding points, "a1" / "a2" the same in float32 (channel sums
    as written / reversed), "ex" the exact float64 step (no rounding points)."""
    kw = dict(head_masks=hm, det_masks=det_masks)
    return dict(ref=pinned_oracle_grads(sd, x, y, draws, masks, bf16=True, **kw),
                a1=pinned_oracle_grads(sd, x, y, draws, masks, bf16=True, dtype=torch.float32, **kw),
                a2=pinned_oracle_grads(sd, x, y, draws, masks, bf16="reversed", dtype=torch.float32, **kw),
                ex=pinned_oracle_grads(sd, x, y, draws, masks, **kw))


def restatement_as_device(triple):
    """A pinned oracle step in the form check_bf16_step takes for the device."""
    g, l, res = triple
    return dict(final=res["out"]["anomaly_scores"].detach().double().numpy(),
                probs=res["out"]["direct_predictions"].detach().double().numpy(), total=float(l["total"]),
                grads={n: (None if t is None else t.detach().double().numpy().reshape(-1)) for n, t in g.items()})


F32_SPREAD = 4.0  # the fp32 step: BF16_SPREAD between two correct fp32 summation orders, times the 2 x that
#                   test_conv3x3_split_accuracy_matches_f32 grants the split-bf16 kernels over exact-f32 MFMA


def f32_step_references(sd, x, y, draws, masks, hm, det_masks=None, stem_pins=None):
    """The pinned oracle steps an fp32 step is judged by, in bf16_step_references' form: "ref" (and "ex", the same
    step) the exact float64 step, "a1" / "a2" the exact path in float32, channel sums as written / reversed."""
    kw = dict(head_masks=hm, det_masks=det_masks, stem_pins=stem_pins)
    ref = pinned_oracle_grads(sd, x, y, draws, masks, **kw)
    return dict(ref=ref, ex=ref, a1=pinned_oracle_grads(sd, x, y, draws, masks, dtype=torch.float32, **kw),
                a2=pinned_oracle_grads(sd, x, y, draws, masks, dtype=torch.float32, reverse_channels=True, **kw))


def check_bf16_step(dev, refs, masks, hm, draws, label, yards=("a1", "a2"), det_hm=None, spread=BF16_SPREAD,
                    grad_floor=1e-5, near=2.0 ** -8, bias_tol=1e-4, mode="bf16"):
    """bf16 parity of one step: dev (final, probs, total, grads {name: flat array}) against the float64 bf16
    restatement refs["ref"], with the float32 restatements named by yards as the yardstick (see BF16_SPREAD) and the
    exact float64 step as a loose backstop.  masks / hm / det_hm: dev's ReLU decisions (backbone, direct classifier,
    detector MLP or None), which every reference was pinned to.  Returns the worst device / yardstick ratio over the
    gradient tensors.
    The defaults are the bf16 mode's bound.  spread: the factor on the yardsticks' distance; grad_floor: the floor of a
    gradient tensor's relative L2 distance; near: a ReLU decision within this fraction of its layer's rms from zero
    may flip on a single rounding; bias_tol: the bound on the pre-BatchNorm biases' gradients (exactly 0); mode: the
    printout's label (the fp32 step: refs of f32_step_references, spread F32_SPREAD, both floors F32_STAT_FLOOR)."""
    from tests.test_oracle_golden import is_pre_bn_bias
    ref_g, ref_l, ref = refs["ref"]
    ys = [refs[k] for k in yards]
    ex_g, ex_l, ex = refs["ex"]
    keep = [torch.from_numpy(draws.direct_keep1), torch.from_numpy(draws.direct_keep2), None, None]
    for i in range(4):
        z = ref["record"][f"dir_z{i}"]
        live = torch.ones_like(hm[i]) if keep[i] is None else keep[i].to(torch.bool)
        fl = ((z > 0) != hm[i]) & live
        rms = float(z.pow(2).mean().sqrt())
        wz = float(z.abs()[fl].max()) if bool(fl.any()) else 0.0
        print(f"  {mode} direct_classifier ReLU {i}: {int(fl.sum())} flips against the float64 restatement "
              f"(worst |z| {wz / rms:.3g} rms)")
        assert wz <= near * rms, i
    if det_hm is not None:
        # the detector MLP's hidden units, pinned the same way; a decision may differ from the float64 restatement's
        # own sign as far as the float32 restatements' own signs do (the backbone layers' rule below)
        keep = [torch.from_numpy(draws.det_keep1), torch.from_numpy(draws.det_keep2), None, None]
        for i in range(4):
            z = ref["record"][f"det_z{i}"]
            live = torch.ones_like(det_hm[i]) if keep[i] is None else keep[i].to(torch.bool)
            fl = ((z > 0) != det_hm[i]) & live
            fas = [((z > 0) != (a[2]["record"][f"det_z{i}"].double() > 0)) & live for a in ys]
            rms = float(z.pow(2).mean().sqrt())
            wz = float(z.abs()[fl].max()) if bool(fl.any()) else 0.0
            wa = max(float(z.abs()[fa].max()) if bool(fa.any()) else 0.0 for fa in fas)
            print(f"  {mode} detector ReLU {i}: {int(fl.sum())} flips against the float64 restatement (worst |z| "
                  f"{wz / rms:.3g} rms; float32 restatements {max(int(fa.sum()) for fa in fas)}, {wa / rms:.3g} rms)")
            assert wz <= spread * wa + near * rms, i
    bad = []

    def within(d, yard, floor, what):
        if not d <= spread * yard + floor:
            bad.append(f"{what}: device {d:.3g} vs float32 restatement {yard:.3g} (bound {spread} x + {floor:g})")

    for key, out_key, floor in (("final", "anomaly_scores", 1e-6), ("probs", "direct_predictions", 1e-6)):
        r64 = ref["out"][out_key].detach().double().numpy()
        d = float(np.abs(dev[key] - r64).max())
        yard = max(float(np.abs(a[2]["out"][out_key].detach().double().numpy() - r64).max()) for a in ys)
        print(f"  {mode} {key}: device {d:.3g}, float32 restatements {yard:.3g}")
        within(d, yard, floor, key)
    d = abs(dev["total"] - float(ref_l["total"]))
    yard = max(abs(float(a[1]["total"]) - float(ref_l["total"])) for a in ys)
    within(d, yard, 1e-6 * abs(float(ref_l["total"])), "total loss")
    # ReLU decisions: the device's (pinned everywhere) against the float64 restatement's own signs, per layer, beside
    # the float32 restatement's own signs
    for l in range(8):
        z64 = ref["record"][f"z{l}"]
        m = masks[l].reshape(z64.shape).to(torch.bool)
        fd = (z64 > 0) != m
        fas = [(z64 > 0) != (a[2]["record"][f"z{l}"].double() > 0) for a in ys]
        wd = float(z64.abs()[fd].max()) if bool(fd.any()) else 0.0
        wa = max(float(z64.abs()[fa].max()) if bool(fa.any()) else 0.0 for fa in fas)
        na = max(int(fa.sum()) for fa in fas)
        rms = float(z64.pow(2).mean().sqrt())
        print(f"  {mode} layer {l} ReLU flips: device {int(fd.sum())} (worst |z| {wd / rms:.3g} rms), float32 "
              f"restatements {na} ({wa / rms:.3g} rms)")
        # (floors: a decision within one bf16 ulp of the layer's scale from zero may flip on a single rounding flip)
        close = int((z64.abs() <= near * rms).sum())
        assert int(fd.sum()) <= spread * na + close, l
        assert wd <= spread * wa + near * rms, l
    worst = 0.0
    for n, mine in dev["grads"].items():
        r = ref_g.get(n)
        if r is None:
            assert mine is None or np.abs(mine).max() == 0.0, n
            continue
        if is_pre_bn_bias(n) or n == "backbone.conv1.bias":  # true gradient 0 (BatchNorm removes the mean)
            assert np.abs(mine).max() < bias_tol, n
            continue
        r = r.detach().double().numpy()
        d = rel_l2(mine, r)
        yard = max(rel_l2(a[0][n].detach().double().numpy(), r) for a in ys)
        exact = rel_l2(mine, ex_g[n].detach().double().numpy())
        worst = max(worst, d / max(yard, 1e-12))
        print(f"  {mode} {n}: device {d:.3g}, float32 restatements {yard:.3g} (device vs the exact step "
              f"{exact:.3g})")
        within(d, yard, grad_floor, n)
        if not exact <= 0.15:
            bad.append(f"{n}: device vs the exact float64 step {exact:.3g} > 0.15 (backstop)")
    for key, out_key in (("final", "anomaly_scores"), ("probs", "direct_predictions")):
        d = float(np.abs(dev[key] - ex["out"][out_key].detach().double().numpy()).max())
        if not d <= 2e-2:
            bad.append(f"{key}: device vs the exact float64 step {d:.3g} > 2e-2 (backstop)")
    if not abs(dev["total"] - float(ex_l["total"])) <= 2e-2 * abs(float(ex_l["total"])):
        bad.append("total loss: device vs the exact float64 step beyond 2e-2 relative (backstop)")
    print(f"{label}, {mode}: worst device / float32-restatements distance ratio {worst:.3g}")
    assert not bad, "; ".join(bad)
    return worst


# ---------------------------------------------------------------- bf16 mode layer by layer, local to the map's edges
BF16_ACT_FLOOR = 2.0 ** -9  # bf16-stored tensors: half a bf16 ulp at the tensor's scale (one rounding flip)
F32_STAT_FLOOR = 1e-6       # the fp32 BatchNorm statistics
MIN_SET = 64                # pixel sets smaller than this are not judged


def _nhwc(t):
    return np.ascontiguousarray(t.detach().double().permute(0, 2, 3, 1).numpy())


def restatement_layer_tensors(triple, masks, store="bf16"):
    """The per-layer tensors of a pinned restatement step as the device stores them (store: "bf16", the bf16 mode's
    storage rounding of dY / dA, or None for the fp32 mode's unrounded ones), {name: float64 array}:
    "pool" and "y{l}" (NF, OH, OW, C); "dY{l}" and "dA{l}" (the gradients of y{l} and of the post-ReLU activation
    a{l}, rounded to bf16 as stored); per channel "mean{l}", "invstd{l}", "mdz{l}" = mean(dZ), "mdzx{l}" =
    mean(dZ * xhat) with dZ = dA{l} masked by the layer's ReLU decision -- taken from the record where a fault
    injection put its own there."""
    from oracle.cad_oracle import bf16r
    if store is None:
        bf16r = lambda t: t  # noqa: E731
    rec = triple[2]["record"]
    out = {"pool": _nhwc(rec["pool_raw"])}
    for l in range(8):
        y = rec[f"y{l}"].detach().double()
        mean = rec[f"mean{l}"].double() if f"mean{l}" in rec else y.mean((0, 2, 3))
        inv = rec[f"invstd{l}"].double() if f"invstd{l}" in rec else torch.rsqrt(y.var((0, 2, 3), unbiased=False) + 1e-5)
        da = bf16r(rec[f"da{l}"]).double()
        dz = da * masks[l].reshape(y.shape).to(torch.float64)
        xh = (y - mean[None, :, None, None]) * inv[None, :, None, None]
        bm = rec.get(f"bwd_means{l}")
        out[f"y{l}"], out[f"dA{l}"], out[f"dY{l}"] = _nhwc(y), _nhwc(da), _nhwc(bf16r(rec[f"dy{l}"]))
        out[f"mean{l}"], out[f"invstd{l}"] = mean.numpy(), inv.numpy()
        out[f"mdz{l}"] = (bm["mdz"].double() if bm else dz.mean((0, 2, 3))).numpy()
        out[f"mdzx{l}"] = (bm["mdzx"].double() if bm else (dz * xh).mean((0, 2, 3))).numpy()
    return out


def device_layer_tensors(eng, run, shapes):
    """The same tensors read from the device after one whole forward + backward of the step.  run() repeats that step
    (called once per layer with the plan's stop_layer debug set, so that layer's dY and the dA under it are still in
    their buffers); shapes: per layer (NF, OH, OW, C).  dA7 (the average pool's backward output) is overwritten inside
    every backward and is not read.  Either storage mode: read_act widens what the plan's last forward stored."""
    from vad_amd import _native as nat
    pl = eng._last[0]
    out = {"pool": read_act(pl, "pool").reshape(shapes[0][:3] + (32,))}  # (layer 0 has stride 1: the pooled map's size)
    for l in range(8):
        C = shapes[l][3]
        st = read_debug(pl, "stats", l + 1).astype(np.float64)
        out[f"y{l}"] = read_act(pl, "y", l).reshape(shapes[l])
        for j, k in ((0, "mean"), (1, "invstd"), (5, "mdz"), (6, "mdzx")):
            out[f"{k}{l}"] = st[j * C:(j + 1) * C]
    try:
        for l in range(7, -1, -1):
            nat.check(nat.lib().vad_cad_set_debug(pl.h, b"stop_layer", l))
            run()
            assert eng._last[0] is pl
            out[f"dY{l}"] = read_act(pl, "dY", 0, n=int(np.prod(shapes[l]))).reshape(shapes[l])
            if l > 0:
                out[f"dA{l - 1}"] = read_act(pl, "dA", 0, n=int(np.prod(shapes[l - 1]))).reshape(shapes[l - 1])
    finally:
        nat.check(nat.lib().vad_cad_set_debug(pl.h, b"stop_layer", -1))
    return out


def local_input_gradients(tens, ref, sd):
    """Each stride's input gradient judged on its own: {"dA{l-1}": ref's dA{l-1} + (tens' dA{l-1} - the float64 input
    gradient of layer l taken from tens' OWN dY{l} and the fp32 weights sd)}, l = 1..7, for check_edge_local against
    ref.  dA{l-1} compared down the whole chain carries the rounding of the forward and of every layer above it (the
    float32 runs: ~1e-6 of its rms), which hides what one input-gradient kernel adds; this residual holds that kernel's
    error alone (the float32 runs: ~2e-7).  fp32 storage only (dY is read as stored)."""
    from oracle.cad_oracle import BACKBONE_CONVS
    out = {}
    for l in range(1, 8):
        if f"dY{l}" not in tens or f"dA{l - 1}" not in tens:
            continue
        conv, _, s = BACKBONE_CONVS[l]
        da = tens[f"dA{l - 1}"]
        dy = torch.from_numpy(np.ascontiguousarray(tens[f"dY{l}"])).permute(0, 3, 1, 2)
        own = torch.nn.grad.conv2d_input((da.shape[0], da.shape[3], da.shape[1], da.shape[2]),
                                         sd[conv + ".weight"].detach().double(), dy, stride=s, padding=1)
        out[f"dA{l - 1}"] = ref[f"dA{l - 1}"] + (da - own.permute(0, 2, 3, 1).numpy())
    return out


def edge_sets(shape, tiles=()):
    """The pixel sets of an (NF, OH, OW, C) map that the edge-local bound is taken over: {label: index}.  tiles:
    (name, NI, TH, TW) of the kernels that tile this map; where the map's edge cuts a tile (or the last frame group is
    partly empty) that tile's last row / column is the map's last one (already a set), and the whole cut strip is
    added.  Sets with the same pixels are listed once."""
    NF, OH, OW, _ = shape
    al = slice(None)
    sets = {"whole": (al, al, al), "first row": (al, slice(0, 1), al), "last row": (al, slice(OH - 1, OH), al),
            "first column": (al, al, slice(0, 1)), "last column": (al, al, slice(OW - 1, OW)),
            "last frame": (slice(NF - 1, NF), al, al)}
    for name, ni, th, tw in tiles:
        if OH % th:
            sets[f"rows of the cut {name} tile"] = (al, slice(OH - OH % th, OH), al)
        if OW % tw:
            sets[f"columns of the cut {name} tile"] = (al, al, slice(OW - OW % tw, OW))
        if NF % ni:
            sets[f"frames of the last {name} group"] = (slice(NF - NF % ni, NF), al, al)
    seen, out = set(), {}
    for k, ix in sets.items():
        key = tuple(s.indices(n) for s, n in zip(ix, (NF, OH, OW)))
        if key not in seen:
            seen.add(key)
            out[k] = ix
    return out


def check_edge_local(dev, ref, yards, tiles, label, quiet=False, spread=BF16_SPREAD, act_floor=BF16_ACT_FLOOR,
                     stat_floor=F32_STAT_FLOOR):
    """The per-layer, edge-local bound (the defaults: the bf16 mode's; the fp32 mode's: spread F32_SPREAD and
    F32_STAT_FLOOR for the maps too).  dev / ref / yards: {name: array} (restatement_layer_tensors /
    device_layer_tensors) of the device, the float64 restatement and the float32 restatements; tiles: {tensor name:
    edge_sets' tiles}.  For every tensor V and pixel set S: E(S) = rms over S of (V - V64) / rms of V64 over the
    whole tensor; the device's must not exceed spread x the largest of the yardsticks' + the floor (act_floor for the
    maps: 2^-9 for bf16-stored ones; stat_floor for the fp32 statistics: 1e-6).  Pixel sets under MIN_SET elements are skipped (printed); a
    statistics vector is one set whatever its channel count: each element is already a mean over every pixel.
    Returns (worst E_dev / max E_f32 over the sets the yardstick moved at all, the failures as strings)."""
    worst, bad = 0.0, []
    for name, v64 in ref.items():
        if name not in dev:
            continue
        scale = max(float(np.sqrt(np.mean(v64 * v64))), 1e-300)
        stat = v64.ndim == 1
        floor = stat_floor if stat else act_floor
        sets = {"whole": (slice(None),)} if stat else edge_sets(v64.shape, tiles.get(name, ()))
        for sname, ix in sets.items():
            r = v64[ix]
            if not stat and r.size < MIN_SET:
                print(f"  {label} {name} [{sname}]: skipped, {r.size} elements")
                continue
            e = float(np.sqrt(np.mean((dev[name][ix] - r) ** 2))) / scale
            ey = max(float(np.sqrt(np.mean((a[name][ix] - r) ** 2))) / scale for a in yards)
            ratio = e / ey if ey > 0 else (0.0 if e == 0 else float("inf"))
            if ey > 0:
                worst = max(worst, ratio)
            if not quiet:
                print(f"  {label} {name} [{sname}]: device {e:.3g}, float32 restatements {ey:.3g}, ratio {ratio:.3g}")
            if not e <= spread * ey + floor:
                bad.append(f"{name} [{sname}]: device {e:.3g} vs float32 restatements {ey:.3g} "
                           f"(bound {spread} x + {floor:.3g})")
    return worst, bad


def check_running_stats(flat_bufs, ref_bufs, rtol=1e-4, atol=1e-5):
    """The engine's flat BN running-stat buffer (library layout) vs {state_dict name: tensor}."""
    from vad_amd import _native as nat
    L = nat.lib()
    fb = flat_bufs.detach().cpu().numpy()
    for i in range(L.vad_cad_num_bufs()):
        n, o, k = L.vad_cad_buf_name(i).decode(), L.vad_cad_buf_offset(i), L.vad_cad_buf_numel(i)
        np.testing.assert_allclose(fb[o:o + k], ref_bufs[n].detach().double().numpy().reshape(-1), rtol=rtol,
                                   atol=atol, err_msg=n)
