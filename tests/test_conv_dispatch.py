"""Which kernel family the backbone's 3x3 convs run on (conv3_choose, csrc/backbone.hip), as vad_cad_conv_path reports
it, pinned against a table recorded from the commit before the chooser existed -- when the launchers, conv3_path,
conv3_act_bf16_ok, conv3_prep_table and conv3_dgrad_w3_wanted each restated the rule in an if-chain of their own.

The table (tests/conv_dispatch_paths.json, which names the commit it was recorded from) holds the 0 / 1 / 2 / 6 code of
every layer (0..7) and pass (forward, input gradient, weight gradient) of plans at SIZES, under every knob setting of
KNOBS, in the three MODES.  vad_cad_create, vad_set_tuning and vad_cad_conv_path touch no device, so this part needs
none.  A mode is set twice: as the calling thread's conv_bf16 / act_bf16 (vad_set_tuning) and as the plan's conv_bf16
option, which is the one vad_cad_conv_path evaluates the rule under.  Regenerate the table with
    python -m tests.test_conv_dispatch --record <commit hash>

DISAGREEMENTS lists the table entries the chooser is meant not to reproduce; there are none: conv3_path agreed with the
launchers on every entry.  Where the other mirrors disagreed with the launchers no path code shows it (the weight
images' layout, below).

The mirrors the plan derives from the same rule are checked on the device at 64 x 64, B T = 2, over the same knob
settings (eval forwards of a trainer-frozen model, fp32 and bf16 compute):
  * bf16 activation storage is chosen exactly when every pass the layers run reports 1 or 2 under bf16 storage;
  * a second forward under unchanged knobs launches no relayout;
  * fp32: flipping conv_patch moves the stride-2 input gradients between the parity-class split kernel and the
    implicit GEMM, whose Wd image is the per-class one: the next forward relayouts;
  * bf16 storage: the native bf16 input gradient reads the bf16 copy whatever conv_patch says, so the flip launches no
    relayout.  (Before the chooser the table wrote the per-class f32 Wd image, which no kernel read, and relayouted.)
"""
import contextlib
import io
import json
import os
import sys

import pytest

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_dispatch_paths.json")
# (B, T, H, W): the frames of test_cad_fp32_ragged_gpu.py / test_cad_bf16_ragged_gpu.py (the first is 227 x 227 at
# B T = 3), 227 x 227 at B T = 32, 64 x 64, and 64 x 64 at B T = 2 (the device part's plan)
SIZES = [(1, 3, 227, 227), (3, 5, 96, 80), (2, 3, 72, 40), (2, 3, 24, 40), (2, 16, 227, 227), (2, 4, 64, 64),
         (2, 1, 64, 64)]
KNOBS = ([{}] +
         [{k: 0} for k in ("conv_patch", "conv_split", "conv_dgrad_s2_x3", "conv_wgrad_tr", "conv_wgrad_split",
                           "conv_wgrad_split_s2")] +
         [{"conv_wgrad_patch": 0}, {"conv_wgrad_patch": 2}, {"conv_patch": 0, "conv_split": 0}])
MODES = {"fp32": (0, 0), "bf16": (1, 0), "bf16_act": (1, 1)}  # (conv_bf16, act_bf16)
# {table key: (code string the chooser gives instead, reason)}
DISAGREEMENTS = {}


def _lib():
    from vad_amd import _native as nat
    return nat, nat.lib()


@contextlib.contextmanager
def knobs(settings):
    """Set tuning knobs (process-global; conv_bf16 / act_bf16: the calling thread's) and put the old values back."""
    import ctypes
    nat, L = _lib()
    old = {}
    try:
        for k, v in settings.items():
            o = ctypes.c_int()
            nat.check(L.vad_get_tuning(k.encode(), ctypes.byref(o)))
            old[k] = o.value
            nat.check(L.vad_set_tuning(k.encode(), v))
        yield
    finally:
        for k, v in old.items():
            nat.check(L.vad_set_tuning(k.encode(), v))


def _key(size, mode, kn):
    return "x".join(map(str, size)) + "|" + mode + "|" + (",".join(f"{k}={v}" for k, v in kn.items()) or "default")


def plan_paths(h, skip_l0_dgrad=False):
    """The 24 codes of a plan, layer-major, (forward, input gradient, weight gradient) per layer."""
    nat, L = _lib()
    return [L.vad_cad_conv_path(h, l, kind) for l in range(8) for kind in range(3)
            if not (skip_l0_dgrad and l == 0 and kind == 1)]


def sweep():
    """{key: the 24 codes as a string} over SIZES x MODES x KNOBS."""
    import ctypes
    nat, L = _lib()
    out = {}
    for size in SIZES:
        h = ctypes.c_void_p()
        nat.check(L.vad_cad_create(*size, ctypes.byref(h)))
        try:
            for mode, (cbf, abf) in MODES.items():
                nat.check(L.vad_cad_set_option(h, b"conv_bf16", cbf))
                for kn in KNOBS:
                    with knobs(dict(kn, conv_bf16=cbf, act_bf16=abf)):
                        out[_key(size, mode, kn)] = "".join(map(str, plan_paths(h)))
        finally:
            L.vad_cad_destroy(h)
    return out


def test_paths_equal_recorded_table():
    with open(TABLE) as f:
        rec = json.load(f)
    want = dict(rec["paths"])
    assert len(rec["parent"]) == 40 and len(want) == len(SIZES) * len(MODES) * len(KNOBS)
    assert set(DISAGREEMENTS) <= set(want)
    for k, (codes, _reason) in DISAGREEMENTS.items():
        assert want[k] != codes, k
        want[k] = codes
    got = sweep()
    assert got.keys() == want.keys()
    bad = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not bad, bad
    # the table is no constant: every code occurs, and the knobs move it
    assert set("".join(want.values())) == set("0126")
    assert len({want[_key(SIZES[0], "fp32", kn)] for kn in KNOBS}) >= 5


def test_knobs_are_restored():
    import ctypes
    nat, L = _lib()
    names = sorted({k for kn in KNOBS for k in kn} | {"conv_bf16", "act_bf16"})

    def read():
        vals = []
        for k in names:
            o = ctypes.c_int()
            nat.check(L.vad_get_tuning(k.encode(), ctypes.byref(o)))
            vals.append(o.value)
        return vals
    before = read()
    sweep()
    assert read() == before


# ---------------------------------------------------------------------------------------------------------------------
# the plan's mirrors, on the device
def _engine(dtype):
    import torch
    from tests.golden_util import make_cad_model
    from vad_amd.train import apply_memory_efficient_training
    m = make_cad_model(dict(seed=1, forced=None))
    with contextlib.redirect_stdout(io.StringIO()):
        apply_memory_efficient_training(m)
    eng = m.cuda().engine()
    eng.compute_dtype = dtype
    return eng


def _forward_relayouts(eng, x):
    """One eval forward; whether it launched the weight relayout (a "prep" record in the plan's profile)."""
    import torch
    eng.profile(True)
    eng.forward(x, False, 0, 0, 0)
    torch.cuda.synchronize()
    labels = eng.profile_read()
    eng.profile(False)
    assert "conv_fwd/L0" in labels
    return "prep" in labels


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_plan_mirrors_follow_the_paths(mode):
    import torch
    from oracle import cad_oracle as co
    from tests.golden_util import read_debug_len
    B, T, H, W = SIZES[-1]
    bf16 = mode == "bf16"
    eng = _engine(torch.bfloat16 if bf16 else torch.float32)
    x = co.synth_clips(1, 0, 0, B, T, H, W).cuda()
    eng.forward(x, False, 0, 0, 0)  # (builds the plan)
    pl = eng.plan(B, T, H, W)
    for kn in KNOBS:
        with knobs(kn):
            _forward_relayouts(eng, x)  # (whatever the setting before left)
            with knobs(dict(act_bf16=1)):  # the rule under bf16 storage (layer 0 runs no input gradient: frozen stem)
                takes_bf16 = all(p in (1, 2) for p in plan_paths(pl.h, skip_l0_dgrad=True))
            assert read_debug_len(pl, "act_bf16") == int(takes_bf16) == int(bf16), kn
            assert not _forward_relayouts(eng, x), kn
            if "conv_patch" not in kn:
                with knobs(dict(conv_patch=0)):
                    assert _forward_relayouts(eng, x) == (not bf16), kn
                    assert not _forward_relayouts(eng, x), kn
                assert _forward_relayouts(eng, x) == (not bf16), kn


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record" and len(sys.argv[2]) == 40, __doc__
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    with open(TABLE, "w") as f:
        json.dump({"parent": sys.argv[2],
                   "codes": "per key B x T x H x W | mode | knobs: vad_cad_conv_path of layers 0..7, (forward, input "
                            "gradient, weight gradient) each",
                   "paths": sweep()}, f, indent=0)
        f.write("\n")
