"""The u8 ingest without a device: vad_ingest_u8 / vad_ingest_u8_table refuse bad arguments on the host, before
anything is queued, naming the argument or the table entry; data.ingest_u8 and the four push_u8 raise their ValueErrors
before any device work."""
import ctypes

import numpy as np
import pytest
import torch

from vad_amd import data
from vad_amd.ae import VideoAutoEncoder
from vad_amd.cad import CausalAnomalyDetector

SRC, DST, TAB = 0x10000, 0x20000, 0x30000  # never dereferenced: every call below is refused first


def _lib():
    from vad_amd import _native
    return _native.lib()


@pytest.mark.parametrize("kw, text", [
    (dict(src=None), "null src"),
    (dict(dst=None), "null dst"),
    (dict(nf=0), "nf must be >= 1"),
    (dict(sh=0), "sh and sw must be >= 1"),
    (dict(sw=0), "sh and sw must be >= 1"),
    (dict(dh=0), "dh and dw must be >= 1"),
    (dict(dw=0), "dh and dw must be >= 1"),
    (dict(dw=4097), "dw must be at most 4096"),
    (dict(sw=9, pitch=8), "pitch 8 is less than sw = 9"),
    (dict(mode=3), "mode 0"),
    (dict(mode=-1), "mode 0"),
    (dict(dst=DST + 4), "dst must be 16-byte aligned"),
    (dict(sh=1 << 16, sw=1 << 15, pitch=1 << 15), "the frame (sh * pitch bytes) is 2 GB or more"),
    (dict(nf=1 << 20, dh=32, dw=16), "dst (nf * dh * dw * 4 bytes) is 2 GB or more"),
    (dict(frame_stride=-1), "frame_stride must be >= 0"),
])
def test_uniform_entry_refuses_before_any_launch(kw, text):
    L = _lib()
    a = dict(src=SRC, nf=2, sh=8, sw=8, pitch=8, frame_stride=64, dh=4, dw=4, mode=0, dst=DST)
    a.update(kw)
    rc = L.vad_ingest_u8(a["src"], a["nf"], a["sh"], a["sw"], a["pitch"], a["frame_stride"], a["dh"], a["dw"],
                         a["mode"], a["dst"], None)
    assert rc == 1
    msg = L.vad_last_error().decode()
    assert msg.startswith("vad_ingest_u8: ") and text in msg, msg


def _table(rows):
    t = np.array(rows, dtype=np.int64).reshape(-1, 4)
    return t, t.ctypes.data


@pytest.mark.parametrize("rows, kw, text", [
    ([(SRC, 8, 8, 8)], dict(host=None), "null table"),
    ([(SRC, 8, 8, 8)], dict(dev=None), "null table"),
    ([(SRC, 8, 8, 8)], dict(dev=TAB + 8), "dev_table must be 16-B aligned"),
    ([(SRC, 8, 8, 8)], dict(dst=None), "null dst"),
    ([(SRC, 8, 8, 8)], dict(dst=DST + 8), "dst must be 16-byte aligned"),
    ([(SRC, 8, 8, 8)], dict(nf=0), "nf must be >= 1"),
    ([(SRC, 8, 8, 8)], dict(dh=0), "dh and dw must be >= 1"),
    ([(SRC, 8, 8, 8)], dict(mode=3), "mode 0"),
    ([(SRC, 8, 8, 8), (0, 0, 0, 0), (SRC, 0, 8, 8)], {}, "entry 2: sh and sw must be >= 1 (got sh = 0, sw = 8)"),
    ([(SRC, 8, 8, 8), (SRC, 8, 0, 8)], {}, "entry 1: sh and sw must be >= 1"),
    ([(0, 0, 0, 0), (SRC, 8, 9, 8)], {}, "entry 1: pitch 8 is less than sw = 9"),
    ([(SRC, 8, 8, 8)] * 3 + [(SRC, 1 << 16, 100, 1 << 15)], {}, "entry 3: the frame (sh * pitch bytes) is 2 GB"),
    ([(SRC, 1 << 40, 8, 8)], {}, "entry 0: the frame (sh * pitch bytes) is 2 GB"),
])
def test_table_entry_refuses_before_any_launch(rows, kw, text):
    L = _lib()
    keep, host = _table(rows)
    a = dict(host=host, nf=len(rows), dh=4, dw=4, mode=2, dst=DST, dev=TAB)
    a.update(kw)
    rc = L.vad_ingest_u8_table(a["host"], a["nf"], a["dh"], a["dw"], a["mode"], a["dst"], a["dev"], None)
    assert rc == 1
    msg = L.vad_last_error().decode()
    assert msg.startswith("vad_ingest_u8_table: ") and text in msg, msg


def test_table_bytes():
    L = _lib()
    assert L.vad_ingest_table_bytes(1) == 32 and L.vad_ingest_table_bytes(96) == 96 * 32
    assert L.vad_ingest_table_bytes(0) < 0
    assert b"vad_ingest_table_bytes" in L.vad_last_error()


def test_u8_to_clip_still_refuses_mode_2():
    L = _lib()
    assert L.vad_u8_to_clip(SRC, 16, 2, DST, None) != 0
    assert b"vad_u8_to_clip: mode 0" in L.vad_last_error()


def _u8(*shape):
    return torch.zeros(*shape, dtype=torch.uint8)


@pytest.fixture
def no_library(monkeypatch):
    """Any use of the library fails the test: the checks under test come before it."""
    def lib():
        raise AssertionError("the library was touched before the argument check")
    monkeypatch.setattr(data.nat, "lib", lib)


@pytest.mark.parametrize("frames, size, mode, text", [
    (torch.zeros(2, 8, 8), (4, 4), 0, "must be uint8"),
    (_u8(8, 8), (4, 4), 0, "shape"),
    (_u8(1, 2, 1, 8, 8), (4, 4), 0, "shape"),
    (_u8(2, 3, 8, 8), (4, 4), 0, "single-channel"),
    (_u8(2, 0, 8), (4, 4), 0, "empty frames"),
    (_u8(0, 8, 8), (4, 4), 0, "no frame"),
    (_u8(2, 8, 8), (4, 0), 0, "size_hw"),
    (_u8(2, 8, 8), (4,), 0, "size_hw"),
    (_u8(2, 8, 8), (4.5, 4), 0, "size_hw"),
    (_u8(2, 8, 8), (4, 4), 3, "mode 0"),
    ([[1, 2]], (4, 4), 0, "shape"),
])
def test_ingest_u8_rejects_bad_arguments(no_library, frames, size, mode, text):
    with pytest.raises(ValueError, match=text):
        data.U8Ingest("cuda:0").ingest(frames, size, mode)
    if isinstance(frames, torch.Tensor) and frames.shape[0] > 0:
        with pytest.raises(ValueError, match=text):
            data.U8Ingest("cuda:0").table([frames], 4, size, mode)
    if text in ("must be uint8", "shape", "single-channel", "empty frames"):
        with pytest.raises(ValueError, match=text):
            data.ingest_u8(frames, size, mode)


def test_ingest_table_rejects_more_frames_than_the_batch(no_library):
    with pytest.raises(ValueError, match="3 frames for a batch of 2"):
        data.U8Ingest("cuda:0").table([_u8(2, 8, 8), _u8(1, 5, 7)], 2, (4, 4), 0)


@pytest.fixture(scope="module")
def cad():
    torch.manual_seed(0)
    return CausalAnomalyDetector().eval()


@pytest.fixture(scope="module")
def ae():
    torch.manual_seed(0)
    return VideoAutoEncoder().eval()


_BAD_SINGLE = [
    (torch.zeros(1, 1, 32, 32), "must be uint8"),
    (_u8(32, 32), "shape"),
    (_u8(1, 1, 1, 32, 32), "shape"),
    (_u8(1, 3, 32, 32), "single-channel"),
    (_u8(3, 32, 32), "between 1 and max_push = 2"),
    (_u8(0, 1, 32, 32), "between 1 and max_push = 2"),
    (_u8(1, 32, 32), "frames on cpu, but the model is on cpu"),  # (a host source needs the model on a HIP device)
]


@pytest.mark.parametrize("frames, text", _BAD_SINGLE)
def test_stream_push_u8_rejects_bad_frames_without_a_device(cad, ae, no_library, frames, text):
    for s in (cad.open_stream(window=4, max_push=2, frame_size=(16, 24)), ae.open_stream(window=4, max_push=2)):
        with pytest.raises(ValueError, match=text):
            s.push_u8(frames)
        assert s.frames_seen == 0 and s.windows_emitted == 0 and s._ring is None and s._ingest is None


_BAD_GROUP = [
    ([_u8(1, 32, 32)], "num_streams = 2 entries"),
    (_u8(2, 32, 32), "num_streams = 2 entries.*got Tensor"),
    ([_u8(1, 32, 32), torch.zeros(1, 32, 32)], "stream 1: frames must be uint8"),
    ([_u8(32, 32), None], "stream 0: .*shape"),
    ([None, _u8(1, 2, 32, 32)], "stream 1: single-channel"),
    ([_u8(3, 32, 32), None], "stream 0: at most max_push = 2 frames per push, got 3"),
    ([None, None], "no stream brought a frame"),
    ([_u8(0, 32, 32), None], "no stream brought a frame"),
    ([_u8(1, 32, 32), _u8(2, 1, 20, 50)], "frames on cpu, but the model is on cpu"),
]


@pytest.mark.parametrize("frames, text", _BAD_GROUP)
def test_group_push_u8_rejects_bad_frames_without_a_device(cad, ae, no_library, frames, text):
    for g in (cad.open_stream_group(2, window=4, max_push=2, frame_size=(16, 24)),
              ae.open_stream_group(2, window=4, max_push=2)):
        with pytest.raises(ValueError, match=text):
            g.push_u8(frames)
        assert g.frames_seen == [0, 0] and g.windows_emitted == [0, 0] and g._ring is None and g._ingest is None


def test_push_u8_rejects_training_mode(cad, ae, no_library):
    streams = [cad.open_stream(window=4), ae.open_stream(window=4)]
    groups = [cad.open_stream_group(1, window=4), ae.open_stream_group(1, window=4)]
    for m in (cad, ae):
        m.train()
    try:
        for s in streams:
            with pytest.raises(ValueError, match="eval mode"):
                s.push_u8(_u8(1, 32, 32))
        for g in groups:
            with pytest.raises(ValueError, match="eval mode"):
                g.push_u8([_u8(1, 32, 32)])
    finally:
        for m in (cad, ae):
            m.eval()


@pytest.mark.parametrize("size", [(0, 8), (8,), (8.5, 8), "ab", 8])
def test_frame_size_keyword_is_checked(cad, size):
    with pytest.raises(ValueError, match="frame_size"):
        cad.open_stream(window=4, frame_size=size)
    with pytest.raises(ValueError, match="frame_size"):
        cad.open_stream_group(2, window=4, frame_size=size)


def test_frame_size_keyword_fixes_the_size_of_fp32_pushes_too(cad):
    s = cad.open_stream(window=4, frame_size=(32, 48))
    assert s.frame_size == (32, 48)
    with pytest.raises(ValueError, match="frame size"):
        s.push(torch.zeros(1, 1, 32, 32))
    g = cad.open_stream_group(2, window=4, frame_size=[32, 48])
    assert g.frame_size == (32, 48)
    with pytest.raises(ValueError, match="frame size"):
        g.push([torch.zeros(1, 1, 32, 32), None])
    assert cad.open_stream(window=4).frame_size is None and cad.open_stream_group(2, window=4).frame_size is None
