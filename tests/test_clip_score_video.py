"""a2 / minicausal score_video and the windows entry points, the parts that need no GPU: every ValueError is raised
before any device work (a valid call on CPU tensors gets as far as the HIP-device check), include/vad.h declares the new
entry points and the library exports them, and the entry points refuse bad window arguments with a text that names the
numbers, before anything is queued (a plan and a fake binding touch no device)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vad_a2_windows_forward", "vad_mc_windows_forward", "vad_bbox_ring_forward")


def a2_model():
    from vad_amd.a2 import CausalAnomalyDetector
    torch.manual_seed(0)
    return CausalAnomalyDetector().eval()


def mc_model(C=1, T=4):
    from vad_amd.mc import SimpleVideoAnomalyDetector
    torch.manual_seed(0)
    return SimpleVideoAnomalyDetector(input_channels=C, temporal_frames=T).eval()


def test_header_declares_and_library_exports_the_windows_entry_points():
    from vad_amd import _native
    src = open(os.path.join(ROOT, "include", "vad.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(vad_\w+)\s*\(", src))
    L = _native.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in _native._SIGS and getattr(L, name).argtypes == _native._SIGS[name][1], name
    # the existing windows call keeps its signature
    assert _native._SIGS["vad_bbox_windows_forward"][1] == [ctypes.c_void_p] * 2 + [ctypes.c_int64] * 3 + [ctypes.c_void_p] * 4


@pytest.mark.parametrize("kind", ["a2", "mc"])
def test_score_video_value_errors_come_before_any_device_work(kind):
    m = a2_model() if kind == "a2" else mc_model(C=1)
    C = 3 if kind == "a2" else 1
    ok = torch.rand(9, C, 10, 13)
    kw = dict(window=4, stride=2, batch=3)
    bad = [
        (dict(frames=torch.rand(9, C, 10)), "frames of shape"),                       # rank
        (dict(frames=torch.rand(9, C + 1, 10, 13)), "frames of shape"),               # channels
        (dict(frames=(ok * 255).to(torch.uint8)), "floating point"),                  # dtype
        (dict(frames=ok.numpy()), "frames of shape"),
        (dict(frames=torch.rand(9, C, 3, 13)), "at least"),                           # too small a frame
        (dict(window=2.5), "window must be an integer"),
        (dict(window=0), "window must be an integer"),
        (dict(window=True), "window must be an integer"),
        (dict(stride=0), "stride must be an integer >= 1"),
        (dict(stride=1.5), "stride must be an integer >= 1"),
        (dict(batch=0), "batch must be an integer >= 1"),
        (dict(batch="4"), "batch must be an integer >= 1"),
        (dict(frames=ok[:3]), "fewer than one window of 4"),
    ]
    if kind == "mc":
        bad.append((dict(window=3), "window must be an integer >= 4"))  # the MaxPool3d stages need T >= 4
    for change, text in bad:
        args = dict(kw, frames=ok)
        args.update(change)
        with pytest.raises(ValueError, match=text):
            m.score_video(**args)
    m.train()
    with pytest.raises(ValueError, match="eval mode"):
        m.score_video(ok, **kw)
    m.eval()
    with pytest.raises(RuntimeError, match="HIP"):  # every check passed: the first device-dependent step refuses
        m.score_video(ok, **kw)
    assert m._engine is None  # nothing was built on the way


def test_mc_window_defaults_to_temporal_frames():
    m = mc_model(C=1, T=6)
    with pytest.raises(ValueError, match="fewer than one window of 6"):
        m.score_video(torch.rand(5, 1, 8, 8))


def test_window_starts_enumerates_the_full_windows():
    from vad_amd.clip_stream import window_starts
    for N, T, s in [(13, 4, 1), (13, 4, 3), (4, 4, 1), (17, 4, 3), (3, 4, 1), (16, 8, 4)]:
        got = window_starts(N, T, s)
        assert got.dtype == torch.int64 and got.tolist() == list(range(0, N - T + 1, s)), (N, T, s)


def _fake_bound(L, prefix, create_args):
    from vad_amd import _native
    h = ctypes.c_void_p()
    _native.check(getattr(L, f"vad_{prefix}_create")(*create_args, ctypes.byref(h)))
    fake = ctypes.c_void_p(256)
    if prefix != "a2":  # (vad_a2_bind copies its offset table to the device; the window checks precede the binding one)
        binds = {"mc": (fake, fake, fake, fake, None, fake, fake, fake), "bbox": (fake, fake)}[prefix]
        _native.check(getattr(L, f"vad_{prefix}_bind")(h, *binds))  # stores pointers only
    return h, fake


@pytest.mark.parametrize("prefix", ["a2", "mc", "bbox"])
def test_windows_entry_points_refuse_before_any_launch(prefix):
    """B = 3 clips of T = 4 frames.  Linear video of 13 frames: the last window must end inside it.  Ring of 6 slots:
    ring >= T, ring <= the buffer, and (nw - 1) * stride + T <= ring so no window of the call laps another."""
    from vad_amd import _native
    L = _native.lib()
    B, T = 3, 4
    h, fake = _fake_bound(L, prefix, {"a2": (B, T, 10, 13), "mc": (B, 1, T, 10, 13), "bbox": (B, T, 10, 13)}[prefix])
    who = {"a2": b"vad_a2_windows_forward", "mc": b"vad_mc_windows_forward", "bbox": b"vad_bbox_ring_forward"}[prefix]

    def call(n_frames=13, first=0, stride=1, ring=0, nw=B, frames=fake, plan=h):
        if prefix == "a2":
            return L.vad_a2_windows_forward(plan, frames, n_frames, first, stride, ring, nw, fake, fake, fake, None)
        if prefix == "mc":
            return L.vad_mc_windows_forward(plan, frames, n_frames, first, stride, ring, nw, fake, None)
        return L.vad_bbox_ring_forward(plan, frames, n_frames, first, stride, ring, fake, fake, fake, None)

    try:
        cases = [
            (dict(plan=None), b": null argument"),
            (dict(frames=None), b": null argument"),
            (dict(stride=0), b": stride must be >= 1, got 0"),
            (dict(first=-1), b": first must be >= 0, got -1"),
            (dict(ring=-2), b": ring must be >= 0"),
            (dict(n_frames=3), b"3 windows of 4 frames from frame 0 at stride 1 end past the video's 3 frames"),
            (dict(first=8), b"from frame 8 at stride 1 end past the video's 13 frames"),    # 8 + 2 + 4 = 14 > 13
            (dict(stride=5), b"at stride 5 end past the video's 13 frames"),                # 10 + 4 = 14 > 13
            (dict(stride=2 ** 62), b"end past the video's 13 frames"),                      # no overflow on the way
            (dict(ring=3, n_frames=6), b"a ring of 3 slots holds no window of 4 frames"),
            (dict(ring=7, n_frames=6), b"a ring of 7 slots in a buffer of 6 frames"),
            (dict(ring=6, n_frames=6, stride=2), b"at stride 2 span more than the ring's 6 slots"),  # 2 * 2 + 4 = 8
        ]
        if prefix != "bbox":  # (bbox runs exactly its plan's B windows)
            cases += [(dict(nw=0), b"between 1 and the plan's 3 windows per call, got 0"),
                      (dict(nw=4), b"between 1 and the plan's 3 windows per call, got 4")]
        for kw, text in cases:
            assert call(**kw) != 0, kw
            assert text in L.vad_last_error() and who in L.vad_last_error(), (kw, L.vad_last_error())
        unbound = ctypes.c_void_p()
        _native.check(getattr(L, f"vad_{prefix}_create")(
            *{"a2": (B, T, 10, 13), "mc": (B, 1, T, 10, 13), "bbox": (B, T, 10, 13)}[prefix], ctypes.byref(unbound)))
        try:
            assert call(plan=unbound) != 0
            assert who + b": plan not bound" in L.vad_last_error()
        finally:
            getattr(L, f"vad_{prefix}_destroy")(unbound)
    finally:
        getattr(L, f"vad_{prefix}_destroy")(h)
