"""The fp32 train step (the split-bf16 kernels of conv_x3.hip / conv_x3w.hip, the BatchNorm sums in their epilogues,
fp32 activation storage) at ragged frame sizes: whole-step bound and a per-layer bound local to the map's edges -- the
fp32 twin of test_cad_bf16_ragged_gpu.py, on the same machinery (tests/golden_util.py).

Instantiations (the fp32 launchers restated by tile_plan below and checked by
test_cases_reach_every_ragged_instantiation).  fwd: "pipe" conv3x3_x3p_kernel<NI,TH,TW> (WCH = 2: 32 input channels,
the weights resident in LDS), "x3" conv3x3_x3_kernel<S,NI,TH,TW,NT>, or path 0 -- conv3_choose (backbone.hip) leaves
the patch kernels for the implicit GEMM where conv3_patch_blocks exceeds NF OH OW / 64; dgrad: stride 1 "x3" conv3x3_x3_kernel with
FWD = false, "fused" where the BnBwdFuse arm (the BatchNorm-backward sums of the layer below) is taken, stride 2 "s2"
conv3x3_dgrad_s2x3_kernel, one frame and 16x16 written pixels per block; wgrad: "tr" x3_wgrad_tr_kernel<S,1,TH,TW,NCO>.
"r:" names the dimensions the map leaves partly empty (h, w; f: the last NI-frame group).  Layer 0 has no input
gradient (frozen stem).

odd227 (NF = 3)
  0 s1 57x57->57x57 | fwd pipe <1,8,32> WCH=2 r:hw | dgrad - | wgrad tr <1,8,16> NCO=1 r:hw
  1 s1 57x57->57x57 | fwd pipe <1,8,32> WCH=2 r:hw | dgrad x3 <1,8,32> fused r:hw | wgrad tr <1,8,16> NCO=1 r:hw
  2 s2 57x57->29x29 | fwd x3 <1,8,32> WCH=1 r:hw | dgrad s2 <1,16,16> fused r:hw | wgrad tr <1,4,16> NCO=2 r:hw
  3 s1 29x29->29x29 | fwd pipe <1,8,32> WCH=1 r:hw | dgrad x3 <1,8,32> fused r:hw | wgrad tr <1,4,16> NCO=2 r:hw
  4 s2 29x29->15x15 | fwd x3 <2,8,16> WCH=1 r:hwf | dgrad s2 <1,16,16> fused r:hw | wgrad tr <1,4,16> NCO=2 r:hw
  5 s1 15x15->15x15 | fwd pipe <2,8,16> WCH=1 r:hwf | dgrad x3 <2,8,16> fused r:hwf | wgrad tr <1,4,16> NCO=2 r:hw
  6 s2 15x15->8x8 | fwd x3 <4,8,8> WCH=1 r:f | dgrad s2 <1,16,16> fused r:hw | wgrad tr <1,8,8> NCO=2 r:-
  7 s1 8x8->8x8 | fwd pipe <4,8,8> WCH=1 r:f | dgrad x3 <4,8,8> fused r:f | wgrad tr <1,8,8> NCO=2 r:-
forced96x80 (NF = 15)
  0 s1 24x20->24x20 | fwd pipe <1,8,32> WCH=2 r:w | dgrad - | wgrad tr <1,8,16> NCO=1 r:w
  1 s1 24x20->24x20 | fwd pipe <1,8,32> WCH=2 r:w | dgrad x3 <1,8,32> fused r:w | wgrad tr <1,8,16> NCO=1 r:w
  2 s2 24x20->12x10 | fwd path 0 (implicit GEMM) | dgrad s2 <1,16,16> fused r:hw | wgrad tr <1,4,16> NCO=2 r:w
  3 s1 12x10->12x10 | fwd path 0 (implicit GEMM) | dgrad x3 <2,8,16> fused r:hwf | wgrad tr <1,4,16> NCO=2 r:w
  4 s2 12x10->6x5 | fwd x3 <4,8,8> WCH=1 r:hwf | dgrad s2 <1,16,16> fused r:hw | wgrad tr <1,8,8> NCO=2 r:hw
  5 s1 6x5->6x5 | fwd pipe <4,8,8> WCH=1 r:hwf | dgrad x3 <4,8,8> fused r:hwf | wgrad tr <1,8,8> NCO=2 r:hw
  6 s2 6x5->3x3 | fwd path 0 (implicit GEMM) | dgrad s2 <1,16,16> fused r:hw | wgrad tr <1,8,8> NCO=2 r:hw
  7 s1 3x3->3x3 | fwd path 0 (implicit GEMM) | dgrad x3 <4,8,8> plain r:hwf | wgrad tr <1,8,8> NCO=2 r:hw
tall72x40 (NF = 6)
  0 s1 18x10->18x10 | fwd path 0 (implicit GEMM) | dgrad - | wgrad tr <1,8,16> NCO=1 r:hw
  1 s1 18x10->18x10 | fwd path 0 (implicit GEMM) | dgrad x3 <2,8,16> fused r:hw | wgrad tr <1,8,16> NCO=1 r:hw
  2 s2 18x10->9x5 | fwd path 0 (implicit GEMM) | dgrad s2 <1,16,16> fused r:hw | wgrad tr <1,8,8> NCO=2 r:hw
  3 s1 9x5->9x5 | fwd path 0 (implicit GEMM) | dgrad x3 <2,8,16> plain r:hw | wgrad tr <1,4,16> NCO=2 r:hw
  4 s2 9x5->5x3 | fwd path 0 (implicit GEMM) | dgrad s2 <1,16,16> fused r:hw | wgrad tr <1,8,8> NCO=2 r:hw
  5 s1 5x3->5x3 | fwd path 0 (implicit GEMM) | dgrad x3 <4,8,8> plain r:hwf | wgrad tr <1,8,8> NCO=2 r:hw
  6 s2 5x3->3x2 | fwd path 0 (implicit GEMM) | dgrad s2 <1,16,16> fused r:hw | wgrad tr <1,8,8> NCO=2 r:hw
  7 s1 3x2->3x2 | fwd path 0 (implicit GEMM) | dgrad x3 <4,8,8> plain r:hwf | wgrad tr <1,8,8> NCO=2 r:hw
small24x40 (NF = 6)
  0 s1 6x10->6x10 | fwd pipe <2,8,16> WCH=2 r:hw | dgrad - | wgrad tr <1,8,16> NCO=1 r:hw
  1 s1 6x10->6x10 | fwd pipe <2,8,16> WCH=2 r:hw | dgrad x3 <2,8,16> plain r:hw | wgrad tr <1,8,16> NCO=1 r:hw
  2 s2 6x10->3x5 | fwd path 0 (implicit GEMM) | dgrad s2 <1,16,16> fused r:hw | wgrad tr <1,8,8> NCO=2 r:hw
  3 s1 3x5->3x5 | fwd path 0 (implicit GEMM) | dgrad x3 <4,8,8> plain r:hwf | wgrad tr <1,8,8> NCO=2 r:hw
  4 s2 3x5->2x3 | fwd path 0 (implicit GEMM) | dgrad s2 <1,16,16> fused r:hw | wgrad tr <1,8,8> NCO=2 r:hw
  5 s1 2x3->2x3 | fwd path 0 (implicit GEMM) | dgrad x3 <4,8,8> plain r:hwf | wgrad tr <1,8,8> NCO=2 r:hw
  6 s2 2x3->1x2 | fwd path 0 (implicit GEMM) | dgrad s2 <1,16,16> fused r:hw | wgrad tr <1,8,8> NCO=2 r:hw
  7 s1 1x2->1x2 | fwd path 0 (implicit GEMM) | dgrad x3 <4,8,8> plain r:hwf | wgrad tr <1,8,8> NCO=2 r:hw

Not reached by any affordable case, and the test that covers each instead:
  * the NT = 2 (64 output channels per block) stride-1 forward and input gradient: launched from 512 tile-slices up --
    test_kernels_gpu.py::test_conv3x3_split_accuracy_matches_f32[64-64-128-13-27-1] (forward; the input gradient's
    NT = 2 arm only in the full-size tests of test_cad_gpu.py);
  * the stride-2 input gradient without its fused BN-backward sums: the plan's partial buffer (>= 1024 floats) never
    falls short of 2 Ci tiles at these sizes -- test_kernels_gpu.py::test_conv3x3_dgrad_s2_split_accuracy_matches_f32;
  * the conv3_wgrad_x3 launchers x3_wgrad_tr defers to (maps 256 wide or tensors of 2 GB):
    test_kernels_gpu.py::test_conv3x3_wgrad_split_accuracy_matches_f32 (path 4).
The fp32 stride-2 input gradient has one frame-group width (one frame per block), unlike the bf16 mode's two.

Two bounds per case (tests/golden_util.py: the exact float64 step pinned to the device's ReLU decisions, and
F32_SPREAD = 4.0 x the larger distance of its two float32 runs, channel sums as written / reversed, + 1e-6):
  * the whole step (check_bf16_step with the fp32 parameters): scores, loss, ReLU decisions, every gradient tensor;
  * layer by layer (check_edge_local): pool (the raw pooled conv1 output, as the frozen fused stem stores it), y, the
    BatchNorm statistics (mean, invstd, mean(dZ), mean(dZ xhat)), dY and dA of every backbone layer, over the whole
    tensor, its first / last row and column, its last frame, and the strip of every tile the map's edge cuts; then
    every input gradient on its own (layer_bound: dA{l-1} against the float64 input gradient of the same run's dY{l}),
    same sets, spread and floor -- dA down the whole chain carries ~1e-6 of rounding in the float32 runs themselves.

What each bound sees (test_injected_faults_are_caught prints it; float32 restatement with one fault at layer 1
(stride 1) / layer 2 (stride 2), the same outcome in all four cases unless noted):
  fault           | layer-by-layer bound      | whole-step bound                   | relative L2 1e-4 (test_cad_gpu.py)
  pad_act         | fails 151-186 sets        | fails                              | fails (0.24-1.2)
  phantom_stats   | fails 145-179 sets        | fails                              | fails (0.034-0.28)
  drop_edge       | fails 22-42 sets          | fails                              | fails (0.1-0.63)
  two_planes      | fails 2-42 sets           | passes (fails: tall72x40 layer 1,  | passes (worst 8.4e-6 - 1.4e-5)
                  |                           | small24x40 both layers)            |
  two_planes_bwd  | fails 5-8 sets, all of    | passes                             | passes (worst 4.1e-6 - 5.9e-6)
                  | the own-dY part           |                                    |
So the three ragged-edge faults also fail the old bound at these shapes (few frames: one column is 2-50 % of a map);
a forward that drops its third bf16 plane (3.4-4.1e-6 of the map's rms against the float32 runs' 4.5-7e-7) is what
only the layer-by-layer bound sees.  The same loss confined to the two gradient kernels passes the chain comparison:
it moves dA by 3.5-4.2e-6 of its rms where the float32 runs themselves differ from float64 by 1.0-2.2e-6, a ratio of
1.7-3.5 under the 4.0 granted (and the layer's weight gradient by 4.1-5.9e-6 against 1.6-2.9e-6).  The input gradient
taken from its own dY shows it: 3.3-3.4e-6 against the float32 runs' 1.7-2.4e-7.  The weight-gradient kernels are
held one at a time by test_kernels_gpu.py::test_conv3x3_wgrad_split_accuracy_matches_f32 (2 x the exact-f32 error).
"""
import contextlib
import ctypes
import functools
import io

import numpy as np
import pytest
import torch

from oracle import cad_oracle as co
from tests.golden.cases import FORCED_A
from tests.golden_util import (F32_SPREAD, F32_STAT_FLOOR, check_bf16_step, check_edge_local, f32_step_references,
                               local_input_gradients, make_cad_model, pinned_oracle_grads, rel_l2,
                               restatement_as_device, restatement_layer_tensors)
from tests.test_cad_bf16_ragged_gpu import CHANNELS, layer_maps, ragged

CASES = [
    dict(name="odd227", B=1, T=3, H=227, W=227, seed=1, step=0, forced=None),
    dict(name="forced96x80", B=3, T=5, H=96, W=80, seed=2, step=0, forced=FORCED_A),
    dict(name="tall72x40", B=2, T=3, H=72, W=40, seed=2, step=0, forced=None),
    dict(name="small24x40", B=2, T=3, H=24, W=40, seed=1, step=0, forced=None),
]
IDS = [c["name"] for c in CASES]
FAULT_LAYERS = (1, 2)  # a stride-1 and a stride-2 layer, the largest maps of each kind
STEP = dict(spread=F32_SPREAD, grad_floor=F32_STAT_FLOOR, near=F32_STAT_FLOOR, bias_tol=1e-6, mode="fp32")
EDGE = dict(spread=F32_SPREAD, act_floor=F32_STAT_FLOOR, stat_floor=F32_STAT_FLOOR)
# the reference-only condition: one float32 restatement against the other at the spread of two correct fp32 runs
STEP_REF, EDGE_REF = dict(STEP, spread=2.0), dict(EDGE, spread=2.0)


def _cdiv(a, b):
    return -(-a // b)


def patch_blocks(nf, oh, ow):
    """conv3_patch_blocks (conv_patch.hip): the BatchNorm partial rows of a patch forward."""
    if oh <= 8 and ow <= 8:
        return _cdiv(nf, 2) * _cdiv(oh, 8) * _cdiv(ow, 8)
    return nf * _cdiv(oh, 8) * _cdiv(ow, 16) if ow <= 16 else nf * _cdiv(oh, 4) * _cdiv(ow, 32)


def parts_floats(nf, H, W):
    """The plan's BatchNorm partial buffer (cad_plan.hip), the capacity the fused BN-backward sums are granted."""
    h1, w1 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    cap = max(nf * _cdiv(h1, 6) * 64, 1024, _cdiv(nf * h1 * w1, 64) * 64)
    for l, (_, _, oh, ow, _) in enumerate(layer_maps(H, W)):
        cap = max(cap, _cdiv(nf * oh * ow, 64) * 2 * CHANNELS[l][1], patch_blocks(nf, oh, ow) * 2 * CHANNELS[l][1])
    return cap


def _x3_tile(h, w):
    """dispatch_pipe / dispatch_x3_nt<1> / dispatch_x3<2> (fp32): (NI, TH, TW) of the map the kernel writes."""
    return (4, 8, 8) if h <= 8 and w <= 8 else (2, 8, 16) if w <= 16 else (1, 8, 32)


def tile_plan(NF, H, W):
    """The fp32 launchers restated (the family: conv3_choose of backbone.hip; within it dispatch_x3 / dispatch_pipe
    / conv3_x3_dgrad / conv3_x3_dgrad_s2 of conv_x3.hip, x3_wgrad_tr of conv_x3w.hip, default knobs).  Per layer:
      "fwd":   (kernel, S, NI, TH, TW, NT, WCH), kernel "pipe" (conv3x3_x3p_kernel) or "x3" (conv3x3_x3_kernel);
      "dgrad": None under the frozen stem's layer 0, else (kernel, S, NI, TH, TW, NT, WCH, fused) in pixels of the map
               it writes -- "x3" (stride 1) or "s2" (conv3x3_dgrad_s2x3_kernel: one frame, an 8x8 class tile = 16x16
               pixels); fused: the BnBwdFuse arm (the layer below's BatchNorm-backward sums in the epilogue) is taken;
      "wgrad": ("tr", S, NI, TH, TW, NCO), x3_wgrad_tr_kernel (the conv3_wgrad_x3 launchers it defers to from 256-wide
               maps or 2 GB tensors up are out of every case's reach);
      "path":  (fwd, dgrad, wgrad) as vad_cad_conv_path reports them: 6 = split-bf16, 0 = the implicit-GEMM fallback of
               a forward whose patch grid exceeds the ceil(M / 64) BatchNorm partial rows."""
    cap = parts_floats(NF, H, W)
    plan = []
    for l, (ih, iw, oh, ow, s) in enumerate(layer_maps(H, W)):
        ci, co_ = CHANNELS[l]
        on_patch = patch_blocks(NF, oh, ow) <= _cdiv(NF * oh * ow, 64)
        if s == 2:
            fwd = ("x3", 2) + _x3_tile(oh, ow) + (1, 1)
            nfuse = 2 * ci * NF * _cdiv((ih + 1) // 2, 8) * _cdiv((iw + 1) // 2, 8)
            dgrad = ("s2", 2, 1, 16, 16, 1, 1, cap >= nfuse)
            wgrad = ("tr", 2, 1) + ((8, 8) if ow <= 8 else (4, 16)) + (2 if co_ % 64 == 0 else 1,)
        else:
            nt = 2 if co_ % 64 == 0 and patch_blocks(NF, oh, ow) * (co_ // 64) >= 512 else 1
            if nt == 1 and 16 < ci <= 256:
                fwd = ("pipe", 1) + _x3_tile(oh, ow) + (1, 2 if ci == 32 else 1)
            else:
                fwd = ("x3", 1) + _x3_tile(oh, ow) + (nt, 2 if nt == 1 and ci == 32 else 1)
            dnt = 2 if ci % 64 == 0 and patch_blocks(NF, ih, iw) * (ci // 64) >= 512 else 1
            dgrad = ("x3", 1) + _x3_tile(ih, iw) + (dnt, 2 if dnt == 1 and co_ == 32 else 1,
                                                    min(512, cap // (2 * ci)) >= 64)
            wgrad = ("tr", 1, 1) + ((8, 16) if co_ % 64 else (8, 8) if ow <= 8 and oh <= 8 else (4, 16))
            wgrad += (2 if co_ % 64 == 0 else 1,)
        plan.append(dict(fwd=fwd if on_patch else None, dgrad=dgrad if l > 0 else None, wgrad=wgrad,
                         path=(6 if on_patch else 0, 6, 6)))
    return plan


def tiles_by_tensor(case):
    """{tensor name: [(kernel, NI, TH, TW)]} for edge_sets: y{l} by the forward that writes it, dY{l} by the weight
    gradient that reads it, dA{l-1} by layer l's input gradient that writes it."""
    out = {}
    for l, k in enumerate(tile_plan(case["B"] * case["T"], case["H"], case["W"])):
        if k["fwd"]:
            out[f"y{l}"] = [("forward",) + k["fwd"][2:5]]
        out[f"dY{l}"] = [("weight-gradient",) + k["wgrad"][2:5]]
        if k["dgrad"]:
            out[f"dA{l - 1}"] = [("input-gradient",) + k["dgrad"][2:5]]
    return out


def describe_plan():
    """The header's listing."""
    lines = []
    for c in CASES:
        nf = c["B"] * c["T"]
        lines.append(f"{c['name']} (NF = {nf})")
        for l, ((ih, iw, oh, ow, s), k) in enumerate(zip(layer_maps(c["H"], c["W"]), tile_plan(nf, c["H"], c["W"]))):
            f, d, w = k["fwd"], k["dgrad"], k["wgrad"]
            fs = f"{f[0]} <{f[2]},{f[3]},{f[4]}> WCH={f[6]} r:{ragged(nf, oh, ow, *f[2:5]) or '-'}" \
                if f else "path 0 (implicit GEMM)"
            ds = f"{d[0]} <{d[2]},{d[3]},{d[4]}> {'fused' if d[7] else 'plain'} r:" \
                 f"{ragged(nf, ih, iw, *d[2:5]) or '-'}" if d else "-"
            ws = f"tr <{w[2]},{w[3]},{w[4]}> NCO={w[5]} r:{ragged(nf, oh, ow, *w[2:5]) or '-'}"
            lines.append(f"  {l} s{s} {ih}x{iw}->{oh}x{ow} | fwd {fs} | dgrad {ds} | wgrad {ws}")
    return "\n".join(lines)


def test_cases_reach_every_ragged_instantiation():
    """The coverage the cases are chosen for, computed from the restated launchers: the three pipelined and the three
    stride-2 forward tiles, the three stride-1 input-gradient tiles (the fused BN-backward arm taken and not taken),
    the stride-2 input gradient, the five weight-gradient tiles -- each met with a map that cuts its
    tile, each NI > 1 family with a partly empty last frame group; the resident-weight (WCH = 2) arms; and at least one
    forward that falls back to path 0."""
    seen, fused, paths = {}, {}, set()
    for c in CASES:
        nf = c["B"] * c["T"]
        for (ih, iw, oh, ow, s), k in zip(layer_maps(c["H"], c["W"]), tile_plan(nf, c["H"], c["W"])):
            paths.add(k["path"][0])
            if k["fwd"]:
                f = k["fwd"]
                seen.setdefault(("fwd",) + f[:5], set()).update(ragged(nf, oh, ow, *f[2:5]))
                if f[6] == 2:
                    seen.setdefault(("fwd-resident", f[0]), set()).update(ragged(nf, oh, ow, *f[2:5]))
            w = k["wgrad"]
            seen.setdefault(("wgrad",) + w[:5], set()).update(ragged(nf, oh, ow, *w[2:5]))
            if k["dgrad"]:
                d = k["dgrad"]
                seen.setdefault(("dgrad",) + d[:5], set()).update(ragged(nf, ih, iw, *d[2:5]))
                fused.setdefault(d[0], set()).add(d[7])
                if d[6] == 2:
                    seen.setdefault(("dgrad-resident",), set()).update(ragged(nf, ih, iw, *d[2:5]))
                assert d[5] == 1 and (not k["fwd"] or k["fwd"][5] == 1), "an NT = 2 kernel below 512 tile-slices"
    tiles = [(4, 8, 8), (2, 8, 16), (1, 8, 32)]
    want = ([("fwd", "pipe", 1) + t for t in tiles] + [("fwd", "x3", 2) + t for t in tiles]
            + [("dgrad", "x3", 1) + t for t in tiles] + [("dgrad", "s2", 2, 1, 16, 16)]
            + [("wgrad", "tr") + t for t in ((2, 1, 8, 8), (2, 1, 4, 16), (1, 1, 8, 16), (1, 1, 8, 8), (1, 1, 4, 16))]
            + [("fwd-resident", "pipe"), ("dgrad-resident",)])
    for k in want:
        assert k in seen, f"{k} is not launched by any case"
        assert seen[k] & set("hw"), f"{k} never meets a map that cuts its tile"
        ni = k[3] if len(k) > 3 else 1
        if ni > 1:
            assert "f" in seen[k], f"{k}: no case leaves its last frame group partly empty"
    assert fused["x3"] == {True, False}, fused
    assert paths == {0, 6}
    for c in CASES:  # no case whose last map holds one value per channel over the whole batch
        assert c["B"] * c["T"] * layer_maps(c["H"], c["W"])[-1][2] * layer_maps(c["H"], c["W"])[-1][3] > 1


def _inputs(case):
    B, T = case["B"], case["T"]
    x = co.synth_clips(case["seed"], case["step"], 0, B, T, case["H"], case["W"])
    return (x, co.synth_labels(0, B), co.CadDraws.make(case["seed"], case["step"], 0, B, T),
            make_cad_model(case).state_dict())


def _f32_tensors(triple, masks):
    return restatement_layer_tensors(triple, masks, store=None)


def layer_bound(dev, r64, yards, case, sd, label, quiet=False, **edge):
    """The layer-by-layer bound: check_edge_local on the stored tensors as they stand, then on every input gradient
    taken on its own (local_input_gradients: dA{l-1} against the float64 input gradient of the implementation's own
    dY{l}), same sets, spread and floor.  Returns (worst ratio of the first part, all failures)."""
    tiles = tiles_by_tensor(case)
    worst, bad = check_edge_local(dev, r64, yards, tiles, label, quiet=quiet, **edge)
    _, bad_l = check_edge_local(local_input_gradients(dev, r64, sd), r64,
                                [local_input_gradients(a, r64, sd) for a in yards], tiles, label + " own dY:",
                                quiet=quiet, **edge)
    return worst, bad + ["from its own dY: " + b for b in bad_l]


@functools.lru_cache(maxsize=None)
def _cpu_references(name):
    """The case's references pinned to the exact float64 forward's own ReLU decisions (backbone, direct classifier,
    detector): (inputs, masks, hm, dm, references, their layer tensors)."""
    case = next(c for c in CASES if c["name"] == name)
    x, y, draws, sd = _inputs(case)
    p = {k: v.detach().double().clone() for k, v in sd.items() if "running" not in k and "num_batches" not in k}
    bufs = {k: v.detach().double().clone() for k, v in sd.items() if "running" in k}
    rec = {}
    with torch.no_grad():
        co.cad_forward(p, bufs, x.double(), draws, training=True, record=rec)
    masks = [rec[f"z{l}"] > 0 for l in range(8)]
    hm = [rec[f"dir_z{i}"] > 0 for i in range(4)]
    dm = [rec[f"det_z{i}"] > 0 for i in range(4)]
    refs = f32_step_references(sd, x, y, draws, masks, hm, dm)
    tens = {k: _f32_tensors(refs[k], masks) for k in ("ref", "a1", "a2")}
    return (x, y, draws, sd), masks, hm, dm, refs, tens


@pytest.mark.parametrize("name", IDS)
def test_references_stay_inside_the_bounds(name):
    """The bounds applied to the references alone, at spread 2.0 (two correct fp32 runs): with the float64 forward's
    own ReLU decisions as the masks, each float32 restatement plays the device against the other one as the only
    yardstick, and satisfies every assertion of the whole-step and of the edge-local bound.  (The seeds of CASES are
    the bf16 file's; none had to be changed.)"""
    case = next(c for c in CASES if c["name"] == name)
    (x, y, draws, sd), masks, hm, dm, refs, tens = _cpu_references(name)
    if case["forced"]:
        assert sum(int(d.shape[0]) for fr in refs["ref"][2]["out"]["detections"] for d in fr) > case["B"] * case["T"]
    for dev, yard in (("a1", "a2"), ("a2", "a1")):
        check_bf16_step(restatement_as_device(refs[dev]), refs, masks, hm, draws, f"{name}: {dev} against {yard}",
                        yards=(yard,), det_hm=dm, **STEP_REF)
        worst, bad = layer_bound(tens[dev], tens["ref"], [tens[yard]], case, sd, f"{name} {dev}/{yard}", quiet=True,
                                 **EDGE_REF)
        print(f"{name}: {dev} against {yard}: worst edge-local ratio {worst:.3g}")
        assert not bad, "; ".join(bad)


def _old_bound_passes(grads, ref_g):
    """The suite's earlier bound on this path (test_cad_gpu.py): every gradient tensor within relative L2 1e-4."""
    from tests.test_oracle_golden import is_pre_bn_bias
    worst = 0.0
    for n, r in ref_g.items():
        if r is None or is_pre_bn_bias(n):
            continue
        worst = max(worst, rel_l2(grads[n].detach().double().numpy(), r.detach().double().numpy()))
    return worst <= 1e-4, worst


@pytest.mark.parametrize("kind", co.F32_FAULTS)
@pytest.mark.parametrize("name", IDS)
def test_injected_faults_are_caught(name, kind):
    """The layer-by-layer bound has teeth: the float32 restatement with one fault injected (oracle F32_FAULTS: the
    three ragged-edge faults of the bf16 file, and a split kernel that drops its third bf16 plane in the forward or in
    the two gradients), at a stride-1 and at a stride-2 layer, plays the device and must fail at least one assertion of
    the edge-local bound.  Whether the whole-step bound and the earlier relative-L2 1e-4 bound would have caught it is
    printed (the file header has the table).
    The third plane lost in the two gradient kernels alone (two_planes_bwd) stays inside the bound on dA compared down
    the whole chain -- 3.5-4.2e-6 of its rms where the float32 runs' own distance is 1.0-2.2e-6 -- and fails it on the
    input gradient taken from its own dY (3.1-3.7e-6 against the float32 runs' 1.2-4.7e-7)."""
    case = next(c for c in CASES if c["name"] == name)
    (x, y, draws, sd), masks, hm, dm, refs, tens = _cpu_references(name)
    missed = []
    for layer in FAULT_LAYERS:
        f = pinned_oracle_grads(sd, x, y, draws, masks, dtype=torch.float32, head_masks=hm, det_masks=dm,
                                fault=(kind, layer))
        _, bad = layer_bound(_f32_tensors(f, masks), tens["ref"], [tens["a1"], tens["a2"]], case, sd,
                             f"{name} {kind}@{layer}", quiet=True, **EDGE)
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                check_bf16_step(restatement_as_device(f), refs, masks, hm, draws, name, det_hm=dm, **STEP)
            step = "passes"
        except AssertionError:
            step = "fails"
        old, worst = _old_bound_passes(f[0], refs["ref"][0])
        print(f"{name}: {kind} at layer {layer}: edge-local bound fails {len(bad)} sets "
              f"(first: {bad[0] if bad else None}); whole-step bound {step}; relative-L2 1e-4 bound "
              f"{'passes' if old else 'fails'} (worst {worst:.2g})")
        if not bad:
            missed.append((kind, layer))
    assert not missed, f"faults the edge-local bound let through: {missed}"


def _frozen(m):
    from vad_amd.train import apply_memory_efficient_training
    with contextlib.redirect_stdout(io.StringIO()):
        apply_memory_efficient_training(m)
    return m


def _device_step(case, frozen=True, layers=True, split=True):
    """One fp32 train step of the case on the device against its references (split: on the split-bf16 kernels, the
    default knobs; else every conv must report path 0).  Returns (worst whole-step gradient
    ratio, worst edge-local ratio or None, the edge-local failures)."""
    from tests.golden_util import (device_layer_tensors, hip_relu_masks, hip_stem_pins, read_debug, read_debug_len,
                                   reshape_masks)
    from vad_amd import _native as nat
    B, T, H, W = case["B"], case["T"], case["H"], case["W"]
    NF = B * T
    x, y, draws, sd = _inputs(case)
    m = make_cad_model(case)
    m = (_frozen(m) if frozen else m).cuda().set_compute_dtype(torch.float32)
    eng = m.engine()
    xd, yd = x.cuda(), y.cuda()

    def run():
        o = eng.forward(xd, True, case["seed"], case["step"], 0, yd)
        eng.backward(True)
        torch.cuda.synchronize()
        return o

    o = run()
    gr = eng.grads.cpu().numpy()
    pl = eng._last[0]
    assert read_debug_len(pl, "act_bf16") == 0 and eng.stem_grad_on == (not frozen)
    for l, k in enumerate(tile_plan(NF, H, W)):
        for kind in range(3):
            if kind == 1 and l == 0 and frozen:
                continue
            assert nat.lib().vad_cad_conv_path(pl.h, l, kind) == (k["path"][kind] if split else 0), (l, kind)
    masks = reshape_masks(hip_relu_masks(eng, NF), x.double())
    pins = None if frozen else hip_stem_pins(eng, NF, H, W)
    hm = [torch.from_numpy(read_debug(pl, "dir_h", i).reshape(B, w) > 0) for i, w in enumerate((512, 256, 128, 64))]
    dm = [torch.from_numpy(read_debug(pl, "det_h", i).reshape(NF, w) > 0)
          for i, w in enumerate((512, 256, 128, 64))] if case["forced"] else None
    refs = f32_step_references(sd, x, y, draws, masks, hm, dm, stem_pins=pins)
    if case["forced"]:  # live detections: a detector gradient joins dA at the average pool
        assert sum(int(d.shape[0]) for fr in refs["ref"][2]["out"]["detections"] for d in fr) > NF
    dev = dict(final=o["final"].cpu().numpy(), probs=o["probs"].cpu().numpy(), total=float(o["losses"][4]),
               grads={n: gr[eng.slot_offset[i]:eng.slot_offset[i] + eng.slot_numel[i]].astype(np.float64)
                      for i, n in enumerate(eng.slot_names)})
    if not frozen:
        assert all(np.abs(dev["grads"][n]).max() > 0 for n in ("backbone.conv1.weight", "backbone.bn1.weight"))
    worst = check_bf16_step(dev, refs, masks, hm, draws, case["name"], det_hm=dm, **STEP)
    if not layers:
        return worst, None, []
    shapes = [(NF, oh, ow, CHANNELS[l][1]) for l, (_, _, oh, ow, _) in enumerate(layer_maps(H, W))]
    devt = device_layer_tensors(eng, run, shapes)
    r64, y1, y2 = (_f32_tensors(refs[k], masks) for k in ("ref", "a1", "a2"))
    worst_e, bad = layer_bound(devt, r64, [y1, y2], case, sd, case["name"], **EDGE)
    print(f"{case['name']}: worst whole-step gradient ratio {worst:.3g}, worst edge-local ratio {worst_e:.3g}")
    return worst, worst_e, bad


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp32_step_at_ragged_sizes(case):
    """One fp32 train step per ragged case on the device (trainer-frozen stem): every layer on the path tile_plan
    restates (vad_cad_conv_path), the whole-step bound (scores, loss, every gradient tensor, the ReLU flip rule)
    against the exact float64 step pinned to the device's decisions, then the per-layer, edge-local bound on pool, y,
    the BatchNorm statistics, dY and dA of all eight layers (dY / dA read from reruns with the plan's stop_layer debug
    set) -- both at F32_SPREAD x the larger distance of the two float32 runs + 1e-6.
    Measured (first run, MI355X): worst gradient ratio device / float32 runs 2.75 (odd227), 1.54 (forced96x80), 3.78
    (tall72x40), 2.5 (small24x40), each where the device is under the 1e-6 floor; worst edge-local ratio 4.54 / 2.74 /
    2.98 / 2.05, every time invstd of layer 0 (device 5-9e-8 of its rms, the float32 runs 2-4e-8: under the floor).
    The input gradients from their own dY: the device's largest residual 8.1e-7 of rms (odd227 dA6, 2304-term sums;
    the float32 runs 2.2e-7), largest ratio 3.9 (dA6 [last column], 6.1e-7: under the floor).  No assertion failed."""
    _, _, bad = _device_step(case)
    assert not bad, "; ".join(bad)


@pytest.mark.gpu
def test_fp32_step_odd227_on_the_exact_f32_kernels():
    """The diagnostic leg: odd227 once more on the exact-f32 MFMA patch kernels (conv_split = 0, the weight gradients
    on the f32 LDS-patch kernel for both strides), same bounds -- a failure of the test above that this leg does not
    share lies in the split numerics, one it shares in the edge handling around them (BatchNorm sums, finalize, apply).
    Measured (first run, MI355X): worst gradient ratio 2.75, worst edge-local ratio 3.4 (invstd of layer 0, under
    the floor); no assertion failed on either leg."""
    from vad_amd import _native as nat
    knobs = {b"conv_split": 0, b"conv_wgrad_patch": 2, b"conv_wgrad_split": 0, b"conv_wgrad_split_s2": 0,
             b"conv_wgrad_tr": 0}
    old = {}
    for k in knobs:
        v = ctypes.c_int()
        nat.check(nat.lib().vad_get_tuning(k, ctypes.byref(v)))
        old[k] = v.value
    try:
        for k, v in knobs.items():
            nat.check(nat.lib().vad_set_tuning(k, v))
        _, _, bad = _device_step(dict(CASES[0], name="odd227 exact-f32 kernels"), split=False)
    finally:
        for k, v in old.items():
            nat.check(nat.lib().vad_set_tuning(k, v))
    assert not bad, "; ".join(bad)


@pytest.mark.gpu
def test_fp32_step_tall72x40_stem_trains():
    """tall72x40 without the trainer's freeze (plan option stem_grad: conv1 / bn1 train, `pool` holds the activated
    map): the whole-step bound only, the stem's ReLU and MaxPool decisions pinned too (hip_stem_pins), with
    backbone.conv1.weight and bn1's gradients among the tensors.
    Measured (first run, MI355X): worst gradient ratio 3.78 (under the floor); no assertion failed."""
    _device_step(dict(CASES[2], name="tall72x40 stem trains"), frozen=False, layers=False)
