"""The colour ingest and the bbox windows without a device: data.luma_u8 against the integer formula and PIL's
convert("L"); vad_ingest_u8_color / vad_ingest_u8_color_table / vad_bbox_windows_forward refuse bad arguments on the
host, before anything is queued, naming the entry point; the Python ValueErrors come before any device work; the clip
enumeration of extract_anomalous_frames."""
import ctypes

import numpy as np
import pytest
import torch

from vad_amd import data
from vad_amd.ae import VideoAutoEncoder
from vad_amd.cad import CausalAnomalyDetector

SRC, DST, TAB = 0x10000, 0x20000, 0x30000  # never dereferenced: every call below is refused first
FORMATS = ("rgb", "bgr", "rgbx", "bgrx")


def _lib():
    from vad_amd import _native
    return _native.lib()


def luma_formula(r, g, b):
    r, g, b = (np.asarray(v).astype(np.int64) for v in (r, g, b))
    return ((r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16).astype(np.uint8)


def pack(rgb: np.ndarray, color: str, rng=None) -> np.ndarray:
    """(..., 3) RGB -> the packed layout of `color`; the X byte of a 4-byte format is noise from rng (or 0)."""
    chans = [rgb[..., 0], rgb[..., 1], rgb[..., 2]]
    if color.startswith("bgr"):
        chans = chans[::-1]
    if len(color) == 4:
        x = rng.integers(0, 256, rgb.shape[:-1], dtype=np.uint8) if rng is not None else np.zeros_like(chans[0])
        chans.append(x)
    return np.ascontiguousarray(np.stack(chans, axis=-1))


def images():
    """An exhaustive (R, G) sweep at several B, a random image and the two extremes, as (Hs, Ws, 3) RGB arrays."""
    r, g = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    out = [np.stack([r, g, np.full_like(r, b)], axis=-1) for b in (0, 1, 37, 127, 128, 200, 254, 255)]
    out.append(np.random.default_rng(0).integers(0, 256, (37, 53, 3), dtype=np.uint8))
    out.append(np.zeros((3, 5, 3), dtype=np.uint8))
    out.append(np.full((3, 5, 3), 255, dtype=np.uint8))
    return out


@pytest.mark.parametrize("color", FORMATS)
def test_luma_u8_is_the_integer_formula(color):
    rng = np.random.default_rng(1)
    for rgb in images():
        want = luma_formula(rgb[..., 0], rgb[..., 1], rgb[..., 2])
        a = pack(rgb, color, rng)
        got = data.luma_u8(a, color)
        assert got.dtype == np.uint8 and got.shape == rgb.shape[:2]
        assert np.array_equal(got, want)
        if len(color) == 4:  # other noise in the X byte: nothing changes
            b = a.copy()
            b[..., 3] = rng.integers(0, 256, b.shape[:2], dtype=np.uint8)
            assert np.array_equal(data.luma_u8(b, color), want)
    assert data.luma_u8(pack(np.zeros((1, 1, 3), np.uint8), color), color)[0, 0] == 0
    assert data.luma_u8(pack(np.full((1, 1, 3), 255, np.uint8), color), color)[0, 0] == 255


@pytest.mark.parametrize("color", FORMATS)
def test_luma_u8_is_pil_convert_l(color):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(2)
    for rgb in images():
        want = np.asarray(Image.fromarray(rgb).convert("L"))
        assert np.array_equal(data.luma_u8(pack(rgb, color, rng), color), want)


@pytest.mark.parametrize("color", FORMATS)
def test_luma_u8_batches_strided_rows_and_torch_input(color):
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, (3, 9, 11, 3), dtype=np.uint8)
    want = luma_formula(rgb[..., 0], rgb[..., 1], rgb[..., 2])
    a = pack(rgb, color, rng)
    step = a.shape[-1]
    assert np.array_equal(data.luma_u8(a, color), want)
    assert np.array_equal(data.luma_u8(torch.from_numpy(a), color), want)
    wide = rng.integers(0, 256, (3, 9, 11 + 4, step), dtype=np.uint8)  # rows pitch = step * (Ws + 4) apart
    wide[:, :, :11] = a
    view = wide[:, :, :11]
    assert view.strides[1] == step * 15 and not view.flags.c_contiguous
    assert np.array_equal(data.luma_u8(view, color), want)
    assert np.array_equal(data.luma_u8(view[1], color), want[1])
    # the C entry itself on the strided rows of one frame
    dst = np.zeros((9, 11), dtype=np.uint8)
    assert _lib().vad_luma_u8(wide[2].ctypes.data, 9, 11, step * 15, FORMATS.index(color), dst.ctypes.data) == 0
    assert np.array_equal(dst, want[2])
    # channels that are not packed go through a copy and agree
    planar = np.ascontiguousarray(a.transpose(0, 3, 1, 2))
    assert np.array_equal(data.luma_u8(planar.transpose(0, 2, 3, 1), color), want)


def test_luma_u8_rejects_bad_arguments():
    L = _lib()
    buf = np.zeros(64, dtype=np.uint8)
    p = buf.ctypes.data
    for args, text in [((None, 2, 2, 6, 0, p), "bad arguments"), ((p, 2, 2, 6, 0, None), "bad arguments"),
                       ((p, 0, 2, 6, 0, p), "bad arguments"), ((p, 2, 2, 6, 4, p), "fmt 0"),
                       ((p, 2, 2, 5, 0, p), "pitch 5 is less than 3 * sw = 6"),
                       ((p, 2, 2, 7, 3, p), "pitch 7 is less than 4 * sw = 8")]:
        assert L.vad_luma_u8(*args) == 1
        msg = L.vad_last_error().decode()
        assert msg.startswith("vad_luma_u8: ") and text in msg, msg
    for frames, color, text in [(np.zeros((4, 4, 3), np.uint8), "gray", "color must be"),
                                (np.zeros((4, 4, 3), np.uint8), "rgbx", "uint8 frames"),
                                (np.zeros((4, 4, 3), np.float32), "rgb", "uint8 frames"),
                                (np.zeros((4, 3), np.uint8), "rgb", "uint8 frames")]:
        with pytest.raises(ValueError, match=text):
            data.luma_u8(frames, color)


_COLOR_REFUSALS = [
    (dict(src=None), "null"),
    (dict(dst=None), "null dst"),
    (dict(fmt=4), "fmt 0 (rgb), 1 (bgr), 2 (rgbx) or 3 (bgrx), got 4"),
    (dict(fmt=-1), "fmt 0"),
    (dict(planes=2), "planes 1 (grey) or 3 (planar RGB), got 2"),
    (dict(planes=0), "planes 1"),
    (dict(sw=8, pitch=23), "pitch 23 is less than 3 * sw = 24"),
    (dict(fmt=1, sw=8, pitch=23), "pitch 23 is less than 3 * sw = 24"),
    (dict(fmt=2, sw=8, pitch=31), "pitch 31 is less than 4 * sw = 32"),
    (dict(fmt=3, sw=8, pitch=31), "pitch 31 is less than 4 * sw = 32"),
    (dict(sh=0), "sh and sw must be >= 1"),
    (dict(nf=0), "nf must be >= 1"),
    (dict(dw=4097), "dw must be at most 4096"),
    (dict(dh=0), "dh and dw must be >= 1"),
    (dict(mode=3), "mode 0"),
    (dict(dst=DST + 4), "dst must be 16-byte aligned"),
    (dict(nf=1 << 19, planes=3, dh=32, dw=16), "dst (nf * planes * dh * dw * 4 bytes) is 2 GB or more"),
    (dict(sh=1 << 16, sw=1 << 13, pitch=1 << 15), "the frame (sh * pitch bytes) is 2 GB or more"),
]


@pytest.mark.parametrize("kw, text", _COLOR_REFUSALS)
def test_color_uniform_entry_refuses_before_any_launch(kw, text):
    L = _lib()
    a = dict(src=SRC, nf=2, sh=8, sw=8, pitch=32, frame_stride=256, fmt=0, planes=1, dh=4, dw=4, mode=0, dst=DST)
    a.update(kw)
    rc = L.vad_ingest_u8_color(a["src"], a["nf"], a["sh"], a["sw"], a["pitch"], a["frame_stride"], a["fmt"],
                               a["planes"], a["dh"], a["dw"], a["mode"], a["dst"], None)
    assert rc == 1
    msg = L.vad_last_error().decode()
    assert msg.startswith("vad_ingest_u8_color: ") and text in msg, msg


def test_color_uniform_entry_refuses_a_negative_frame_stride():
    L = _lib()
    assert L.vad_ingest_u8_color(SRC, 2, 8, 8, 24, -1, 0, 1, 4, 4, 0, DST, None) == 1
    assert b"vad_ingest_u8_color: frame_stride must be >= 0" in L.vad_last_error()


@pytest.mark.parametrize("kw, text", [(k, t) for k, t in _COLOR_REFUSALS if "src" not in k] + [
    (dict(host=None), "null table"),
    (dict(dev=None), "null table"),
    (dict(dev=TAB + 8), "dev_table must be 16-B aligned"),
])
def test_color_table_entry_refuses_before_any_launch(kw, text):
    """The same violations through the table form: a bad source is the last of three rows, behind a padding row, and
    the error names it as entry 2."""
    L = _lib()
    a = dict(nf=3, sh=8, sw=8, pitch=32, fmt=0, planes=1, dh=4, dw=4, mode=0, dst=DST, dev=TAB)
    a.update(kw)
    rows = [(SRC, 8, 8, 32), (0, 0, 0, 0), (SRC, a["sh"], a["sw"], a["pitch"])]
    if a["nf"] > 3:
        rows = rows[:1]  # (the output check comes first; the table is not read)
    table = np.array(rows, dtype=np.int64)
    host = a.get("host", table.ctypes.data)
    rc = L.vad_ingest_u8_color_table(host, a["nf"], a["fmt"], a["planes"], a["dh"], a["dw"], a["mode"], a["dst"],
                                     a["dev"], None)
    assert rc == 1
    msg = L.vad_last_error().decode()
    assert msg.startswith("vad_ingest_u8_color_table: ") and text in msg, msg
    if {"sh", "sw", "pitch"} & set(kw):
        assert "entry 2: " in msg, msg


def _u8(*shape):
    return torch.zeros(*shape, dtype=torch.uint8)


@pytest.fixture
def no_library(monkeypatch):
    """Any use of the library fails the test: the checks under test come before it."""
    def lib():
        raise AssertionError("the library was touched before the argument check")
    monkeypatch.setattr(data.nat, "lib", lib)


@pytest.mark.parametrize("frames, kw, text", [
    (_u8(2, 8, 8, 3), dict(color="gray"), "color must be"),
    (_u8(2, 8, 8, 3), dict(color=1), "color must be"),
    (_u8(2, 8, 8, 3), dict(color="rgbx"), "4 bytes per pixel"),
    (_u8(2, 8, 8, 4), dict(color="bgr"), "3 bytes per pixel"),
    (_u8(2, 3, 8, 8), dict(color="rgb"), "3 bytes per pixel"),
    (_u8(8, 8, 3), dict(color="rgb"), "shape"),
    (_u8(1, 2, 8, 8, 3), dict(color="rgb"), "shape"),
    (torch.zeros(2, 8, 8, 3), dict(color="rgb"), "must be uint8"),
    (_u8(2, 0, 8, 3), dict(color="rgb"), "empty frames"),
    (_u8(2, 8, 8, 3), dict(color="rgb", planes=2), "planes must be 1"),
    (_u8(2, 8, 8, 3), dict(color="rgb", planes=True), "planes must be 1"),
    (_u8(2, 8, 8), dict(planes=3), "planes=3 needs colour frames"),
    (_u8(2, 8, 8), dict(planes=4), "planes must be 1"),
    (_u8(2, 3, 8, 8), dict(), "single-channel frames only"),       # colour without the keyword: the old error
    (_u8(2, 3, 8, 8), dict(color=None), "single-channel frames only"),
])
def test_ingest_u8_color_rejects_bad_arguments(no_library, frames, kw, text):
    with pytest.raises(ValueError, match=text):
        data.ingest_u8(frames, (4, 4), 0, **kw)
    with pytest.raises(ValueError, match=text):
        data.U8Ingest("cuda:0").ingest(frames, (4, 4), 0, **kw)
    with pytest.raises(ValueError, match=text):
        data.U8Ingest("cuda:0").table([frames], 4, (4, 4), 0, **kw)


def test_ingest_u8_color_still_checks_size_mode_and_count(no_library):
    ing = data.U8Ingest("cuda:0")
    with pytest.raises(ValueError, match="size_hw"):
        ing.ingest(_u8(2, 8, 8, 3), (4, 0), 0, color="rgb")
    with pytest.raises(ValueError, match="mode 0"):
        ing.ingest(_u8(2, 8, 8, 3), (4, 4), 3, color="rgb", planes=3)
    with pytest.raises(ValueError, match="no frame"):
        ing.ingest(_u8(0, 8, 8, 3), (4, 4), 0, color="rgb")
    with pytest.raises(ValueError, match="3 frames for a batch of 2"):
        ing.table([_u8(2, 8, 8, 4), _u8(1, 5, 7, 4)], 2, (4, 4), 0, color="bgrx", planes=3)


@pytest.fixture(scope="module")
def cad():
    torch.manual_seed(0)
    return CausalAnomalyDetector().eval()


@pytest.fixture(scope="module")
def ae():
    torch.manual_seed(0)
    return VideoAutoEncoder().eval()


_BAD_PUSH = [
    (_u8(1, 32, 32, 3), "yuv", "color must be"),
    (_u8(1, 32, 32, 3), "bgrx", "4 bytes per pixel"),
    (_u8(1, 32, 32), "bgr", "shape"),
    (_u8(1, 1, 32, 32), "bgr", "3 bytes per pixel"),
    (torch.zeros(1, 32, 32, 3), "bgr", "must be uint8"),
    (_u8(3, 32, 32, 3), "bgr", "between 1 and max_push = 2"),
    (_u8(1, 32, 32, 3), None, "single-channel"),  # ((k, 32, 32, 3) read as (k, C, Hs, Ws) with 32 channels)
    (_u8(1, 32, 32, 3), "bgr", "frames on cpu, but the model is on cpu"),
]


@pytest.mark.parametrize("frames, color, text", _BAD_PUSH)
def test_stream_push_u8_color_rejects_bad_frames_without_a_device(cad, ae, no_library, frames, color, text):
    for s in (cad.open_stream(window=4, max_push=2, frame_size=(16, 24)), ae.open_stream(window=4, max_push=2)):
        with pytest.raises(ValueError, match=text):
            s.push_u8(frames, color=color)
        assert s.frames_seen == 0 and s.windows_emitted == 0 and s._ring is None and s._ingest is None
    for g in (cad.open_stream_group(2, window=4, max_push=2, frame_size=(16, 24)),
              ae.open_stream_group(2, window=4, max_push=2)):
        with pytest.raises(ValueError, match=text.replace("between 1 and", "at most")):
            g.push_u8([None, frames], color=color)
        assert g.frames_seen == [0, 0] and g.windows_emitted == [0, 0] and g._ring is None and g._ingest is None


def test_bbox_clip_enumeration_is_the_reference_s():
    from vad_amd.bbox import clip_starts
    want = {7: [], 8: [], 9: [0], 12: [0], 13: [0, 4], 16: [0, 4], 17: [0, 4, 8]}
    assert {n: clip_starts(n) for n in want} == want


def test_bbox_windows_forward_refuses_before_any_launch():
    """On a plan that is not bound: the argument checks come first and need no device."""
    from vad_amd import _native
    L = _lib()
    h = ctypes.c_void_p()
    _native.check(L.vad_bbox_create(3, 8, 64, 64, ctypes.byref(h)))  # windows 0, s, 2s of 8 frames
    fake = ctypes.c_void_p(256)
    try:
        def call(plan=h, frames=fake, n=16, first=0, stride=4, scores=fake, adj=fake):
            rc = L.vad_bbox_windows_forward(plan, frames, n, first, stride, scores, adj, None, None)
            return rc, L.vad_last_error().decode()
        for kw in (dict(plan=None), dict(frames=None), dict(scores=None), dict(adj=None)):
            rc, msg = call(**kw)
            assert rc == 1 and msg == "vad_bbox_windows_forward: null argument", msg
        rc, msg = call(stride=0)
        assert rc == 1 and "vad_bbox_windows_forward: stride must be >= 1, got 0" in msg, msg
        rc, msg = call(first=-1)
        assert rc == 1 and "vad_bbox_windows_forward: first must be >= 0, got -1" in msg, msg
        for kw in (dict(n=15), dict(first=1), dict(stride=5), dict(n=7), dict(stride=1 << 62), dict(first=1 << 62)):
            rc, msg = call(**kw)
            assert rc == 1 and msg.startswith("vad_bbox_windows_forward: 3 windows of 8 frames") \
                and "end past the video's" in msg, msg
        rc, msg = call()  # 0, 4, 8 (+ 8) in 16 frames: legal, and stops at the binding
        assert rc == 1 and msg == "vad_bbox_windows_forward: plan not bound", msg
    finally:
        L.vad_bbox_destroy(h)


def test_bbox_score_video_rejects_bad_arguments(no_library):
    from vad_amd.bbox import CausalAnomalyDetector as Bbox
    torch.manual_seed(0)
    m = Bbox().eval()
    x = torch.zeros(16, 3, 8, 8)
    for frames, kw, text in [(torch.zeros(7, 3, 8, 8), {}, "7 frames, fewer than one window of 8"),
                             (torch.zeros(16, 1, 8, 8), {}, r"\(N, 3, H, W\)"),
                             (torch.zeros(1, 16, 3, 8, 8), {}, r"\(N, 3, H, W\)"),
                             (torch.zeros(16, 3, 8, 8, dtype=torch.uint8), {}, "floating point"),
                             (torch.zeros(16, 3, 1, 8), {}, "at least 2 x 2"),
                             (x, dict(window=1), "window must be an integer >= 2"),
                             (x, dict(window=2.5), "window must be"),
                             (x, dict(stride=0), "stride must be an integer >= 1"),
                             (x, dict(batch=0), "batch must be an integer >= 1"),
                             (x, dict(batch=True), "batch must be")]:
        with pytest.raises(ValueError, match=text):
            m.score_video(frames, **kw)
    m.train()
    with pytest.raises(ValueError, match="eval mode"):
        m.score_video(x)
