"""The colour ingest on the GPU.  The yardstick is the host route -- data.luma_u8 at the source size (or the channel
itself for planes=3), data.resize_u8, the float32 numpy expression of the mode -- never the kernel under test, and
every comparison is exact (np.array_equal / torch.equal): the arithmetic is integer up to one float operation per
pixel."""
import numpy as np
import pytest
import torch

from tests.golden_util import make_cad_model
from tests.test_ae_score_video_gpu import make_model as make_ae_model
from tests.test_ingest_gpu import _same_dicts, assert_bits, host_ingest, normalise
from vad_amd import data

pytestmark = pytest.mark.gpu

FORMATS = ("rgb", "bgr", "rgbx", "bgrx")
OUTPUTS = [(1, 0), (1, 2), (3, 1)]  # (planes, mode)


def rgb_of(src: np.ndarray, color: str):
    r = 2 if color.startswith("bgr") else 0
    return src[..., r], src[..., 1], src[..., 2 - r]


def host_color(src: np.ndarray, color: str, size, mode: int, planes: int) -> np.ndarray:
    """(k, Hs, Ws, C) packed u8 -> (k, planes, H, W) float32 by the host route."""
    if planes == 1:
        return host_ingest(data.luma_u8(src, color), size, mode)
    chans = [np.ascontiguousarray(c) for c in rgb_of(src, color)]
    out = np.stack([host_ingest(c, size, mode)[:, 0] for c in chans], axis=1)
    assert out.dtype == np.float32 and out.shape == (src.shape[0], 3, *size)
    return out


def camera(seed, k, hs, ws, color):
    return np.random.default_rng(seed).integers(0, 256, (k, hs, ws, len(color)), dtype=np.uint8)


def guarded(n, k, planes, dh, dw):
    """A NaN-filled buffer whose first k * planes * dh * dw floats are the output; the rest is the guard."""
    buf = torch.full((n + 64,), float("nan"), device="cuda")
    return buf, buf[:n].view(k, planes, dh, dw)


SHAPES = [((7, 9), (5, 13)), ((1, 1), (6, 10)), ((40, 3), (6, 10)), ((9, 1), (5, 13)), ((33, 37), (33, 37)),
          ((12, 20), (64, 64))]


@pytest.mark.parametrize("color", FORMATS)
@pytest.mark.parametrize("src_hw, dst_hw", SHAPES, ids=[f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in SHAPES])
def test_uniform_form_equals_the_host_route(src_hw, dst_hw, color):
    """Four frames -- two random, all-255, all-0 -- so that later frames start unaligned where dh * dw is no multiple
    of 4; from the device and from pinned memory; then a row-strided view (pitch = step * (sw + 3), one byte past an
    aligned address) into an out= with a NaN guard behind it."""
    sh, sw = src_hw
    dh, dw = dst_hw
    step = len(color)
    src = camera(1000 * sh + 10 * sw + step, 4, sh, sw, color)
    src[2] = 255
    src[3] = 0
    t = torch.from_numpy(src)
    flat = torch.zeros(1 + 4 * sh * (sw + 3) * step, dtype=torch.uint8)
    flat[1:].view(4, sh, sw + 3, step)[:, :, :sw].copy_(t)
    strided = flat.cuda()[1:].view(4, sh, sw + 3, step)[:, :, :sw]
    assert strided.data_ptr() % 16 == 1
    for planes, mode in OUTPUTS:
        want = host_color(src, color, dst_hw, mode, planes)
        if src_hw == dst_hw and planes == 3:  # the identity: the channel itself
            assert np.array_equal(want, normalise(np.stack(rgb_of(src, color), axis=1), mode))
        for where, x in (("device", t.cuda()), ("pinned", t.pin_memory())):
            assert_bits(data.ingest_u8(x, dst_hw, mode, color=color, planes=planes), want,
                        f"planes {planes} mode {mode} {where}")
        buf, out = guarded(want.size, 4, planes, dh, dw)
        got = data.ingest_u8(strided, dst_hw, mode, out=out, color=color, planes=planes)
        assert got is out
        assert_bits(out, want, f"planes {planes} mode {mode} strided rows")
        assert torch.isnan(buf[want.size:]).all(), "the guard behind out was written"


@pytest.mark.parametrize("planes, mode", OUTPUTS)
@pytest.mark.parametrize("color", ["bgr", "rgbx"])
def test_table_form_mixed_sizes_padding_and_guard(color, planes, mode):
    """Three chunks of three source sizes -- pinned, pageable, device -- and two padding frames: padding is exactly zero
    in every plane, the others equal the host route, the guard behind the frames stays NaN."""
    dh, dw = 5, 13
    srcs = [camera(7, 2, 9, 14, color), camera(8, 1, 40, 3, color), camera(9, 2, 4, 5, color)]
    t = [torch.from_numpy(s) for s in srcs]
    chunks = [t[0].pin_memory(), t[1], t[2].cuda()]
    n = 7
    buf, out = guarded(n * planes * dh * dw, n, planes, dh, dw)
    ing = data.U8Ingest(torch.device("cuda", torch.cuda.current_device()))
    got = ing.table(chunks, n, (dh, dw), mode, out=out, color=color, planes=planes)
    assert got is out
    want = np.concatenate([host_color(s, color, (dh, dw), mode, planes) for s in srcs])
    assert_bits(out[:5], want, "frames")
    assert torch.equal(out[5:], torch.zeros(2, planes, dh, dw, device="cuda")), "padding frames"
    assert torch.isnan(buf[n * planes * dh * dw:]).all(), "the guard behind the frames was written"
    # the same object again, without padding and with another format of the same step (the tables are reused)
    other = {"bgr": "rgb", "rgbx": "bgrx"}[color]
    again = ing.table(chunks[::-1], 5, (dh, dw), mode, color=other, planes=planes)
    want = np.concatenate([host_color(s, other, (dh, dw), mode, planes) for s in srcs[::-1]])
    assert_bits(again, want, "second launch")


def test_sources_pinned_pageable_device_and_views_that_need_a_copy():
    rgb = camera(21, 3, 11, 19, "rgb")
    t = torch.from_numpy(rgb)
    for planes, mode in OUTPUTS:
        want = host_color(rgb, "rgb", (6, 10), mode, planes)
        for where, x in (("pinned", t.pin_memory()), ("pageable", t), ("device", t.cuda())):
            assert_bits(data.ingest_u8(x, (6, 10), mode, color="rgb", planes=planes), want, where)
            # the channels reversed are the same picture in the other order
            assert_bits(data.ingest_u8(x.flip(-1), (6, 10), mode, color="bgr", planes=planes), want,
                        f"{where}, flipped")
        # channels that are not packed (a planar tensor seen as (k, Hs, Ws, 3)): made contiguous first
        planar = t.permute(0, 3, 1, 2).contiguous()
        for where, x in (("pinned", planar.pin_memory()), ("device", planar.cuda())):
            view = x.permute(0, 2, 3, 1)
            assert view.stride(3) != 1
            assert_bits(data.ingest_u8(view, (6, 10), mode, color="rgb", planes=planes), want, f"{where}, planar view")
    # the first three bytes of 4-byte pixels read as "rgb": pixels are 4 apart, not 3 -> a copy, and the same result
    x4 = torch.from_numpy(camera(22, 2, 7, 9, "rgbx")).cuda()
    assert torch.equal(data.ingest_u8(x4[..., :3], (5, 13), 0, color="rgb"), data.ingest_u8(x4, (5, 13), 0, color="rgbx"))


PUSHES = [3, 2, 3, 3]  # 11 frames on a ring of window + max_push - 1 = 6 slots: it wraps


def host_grey_frames(src, color, size, mode):
    return torch.from_numpy(host_color(src, color, size, mode, 1)).cuda()


@pytest.mark.parametrize("frame_size", [(24, 36), None], ids=["resize", "identity"])
def test_cad_stream_push_u8_colour_is_push_on_host_built_frames(frame_size):
    m = make_cad_model(dict(name="color_ingest", seed=3, forced=None)).cuda().eval()
    u8 = camera(31, sum(PUSHES), 30, 50, "bgr")
    x = host_grey_frames(u8, "bgr", frame_size or (30, 50), 0)
    kw = dict(window=4, stride=1, max_push=3, seed=5, clip0=1)
    ref, s = m.open_stream(**kw), m.open_stream(frame_size=frame_size, **kw)
    f = windows = 0
    for i, k in enumerate(PUSHES):
        want = ref.push(x[f:f + k])
        src = torch.from_numpy(u8[f:f + k])
        got = s.push_u8((src.pin_memory(), src.cuda(), src)[i % 3], color="bgr")
        _same_dicts(got, want, f"push {i}")
        windows += got["anomaly_scores"].shape[0]
        f += k
    assert s.frame_size == (frame_size or (30, 50)) and s.frames_seen == f == 11 and windows == f - 3


def test_ae_stream_push_u8_colour_is_push_on_host_built_frames():
    m = make_ae_model(46).cuda().eval()
    u8 = camera(32, sum(PUSHES), 48, 80, "rgbx")
    x = host_grey_frames(u8, "rgbx", (64, 64), 2)
    kw = dict(window=4, stride=1, max_push=3, return_reconstructions=True)
    ref, s = m.open_stream(**kw), m.open_stream(**kw)
    f = 0
    for i, k in enumerate(PUSHES):
        want = ref.push(x[f:f + k])
        src = torch.from_numpy(u8[f:f + k])
        _same_dicts(s.push_u8((src.pin_memory(), src.cuda(), src)[i % 3], color="rgbx"), want, f"push {i}")
        f += k
    assert s.frames_seen == f and s.windows_emitted == f - 3


CAMERAS = [(40, 60), (32, 48), (57, 33)]
GROUP_KS = [(2, None, 1), (1, 2, 0), (None, 2, 2), (2, 2, 2), (0, 1, None), (1, None, 2)]


def _group_pushes(g_u8, g_ref, cams, color, size, mode):
    seen = [0, 0, 0]
    for p, ks in enumerate(GROUP_KS):
        u8s, xs = [], []
        for s, k in enumerate(ks):
            if k is None:
                u8s.append(None)
                xs.append(None)
                continue
            chunk = cams[s][seen[s]:seen[s] + k]
            src = torch.from_numpy(chunk)
            u8s.append((src.pin_memory(), src.cuda(), src)[(p + s) % 3] if k else src)
            xs.append(host_grey_frames(chunk, color, size, mode) if k else torch.zeros(0, 1, *size, device="cuda"))
            seen[s] += k
        got, want = g_u8.push_u8(u8s, color=color), g_ref.push(xs)
        assert len(got) == len(want) == 3
        for s in range(3):
            _same_dicts(got[s], want[s], f"push {p} stream {s}")
    assert g_u8.frames_seen == g_ref.frames_seen == seen


def test_cad_group_push_u8_colour_is_push_on_host_built_frames():
    """Three cameras of three source sizes; ks include None, 0 and max_push."""
    m = make_cad_model(dict(name="color_ingest_g", seed=4, forced=None)).cuda().eval()
    cams = [camera(40 + s, 8, *hw, "bgr") for s, hw in enumerate(CAMERAS)]
    kw = dict(window=4, stride=1, max_push=2, seed=2, clip0=[0, 5, 9], frame_size=(24, 36))
    _group_pushes(m.open_stream_group(3, **kw), m.open_stream_group(3, **kw), cams, "bgr", (24, 36), 0)


def test_ae_group_push_u8_colour_is_push_on_host_built_frames():
    m = make_ae_model(46).cuda().eval()
    cams = [camera(50 + s, 8, *hw, "bgrx") for s, hw in enumerate(CAMERAS)]
    kw = dict(window=4, stride=1, max_push=2, return_reconstructions=True)
    _group_pushes(m.open_stream_group(3, **kw), m.open_stream_group(3, **kw), cams, "bgrx", (64, 64), 2)


def test_grey_and_colour_pushes_interleave_on_one_stream():
    """Grey and colour push_u8 calls in turn on one stream equal the undisturbed sequence on host-built frames."""
    m = make_cad_model(dict(name="color_ingest_mix", seed=6, forced=None)).cuda().eval()
    size = (24, 36)
    col = camera(61, 10, 30, 50, "rgb")
    grey = np.random.default_rng(62).integers(0, 256, (10, 41, 29), dtype=np.uint8)
    kw = dict(window=4, stride=1, max_push=2, seed=7, frame_size=size)
    ref, s = m.open_stream(**kw), m.open_stream(**kw)
    f = 0
    for i, k in enumerate([2, 1, 2, 2, 1, 2]):
        if i % 2:
            x = host_grey_frames(col[f:f + k], "rgb", size, 0)
            got = s.push_u8(torch.from_numpy(col[f:f + k]), color="rgb")
        else:
            x = torch.from_numpy(host_ingest(grey[f:f + k], size, 0)).cuda()
            got = s.push_u8(torch.from_numpy(grey[f:f + k]).pin_memory())
        _same_dicts(got, ref.push(x), f"push {i}")
        f += k
    assert s.frames_seen == ref.frames_seen == 10
