"""The u8 ingest on the GPU.  The yardstick everywhere is the host routine data.resize_u8 followed by the float32 numpy
expression of the mode -- never the kernel under test -- and equality is exact: the arithmetic is integer up to one
float operation per pixel, so np.array_equal / torch.equal with no tolerance."""
import numpy as np
import pytest
import torch

from oracle import cad_oracle as co
from tests.golden_util import make_cad_model
from tests.test_ae_score_video_gpu import make_model as make_ae_model
from vad_amd import _native as nat
from vad_amd import data

pytestmark = pytest.mark.gpu

F32 = np.float32


def normalise(u8: np.ndarray, mode: int) -> np.ndarray:
    f = u8.astype(F32)
    if mode == 0:
        return (f - F32(0.5)) / F32(0.5)
    if mode == 1:
        return f / F32(255)
    return np.clip(f / F32(255), F32(0.001), F32(0.999))


def host_ingest(src: np.ndarray, size, mode: int) -> np.ndarray:
    """(k, Hs, Ws) u8 -> (k, 1, H, W) float32 by the host route."""
    out = np.stack([normalise(data.resize_u8(f, *size), mode) for f in src])[:, None]
    assert out.dtype == F32
    return out


def contents(kind, rng, nf, sh, sw):
    if kind == "random":
        return rng.integers(0, 256, (nf, sh, sw), dtype=np.uint8)
    if kind == "white":  # the largest intermediate sums
        return np.full((nf, sh, sw), 255, dtype=np.uint8)
    return ((np.arange(nf * sh * sw) * 7) % 256).astype(np.uint8).reshape(nf, sh, sw)  # ramp


def assert_bits(got: torch.Tensor, want: np.ndarray, what):
    g = got.cpu().numpy()
    assert g.shape == want.shape and g.dtype == want.dtype, what
    if not np.array_equal(g, want):
        bad = np.argwhere(g != want)
        raise AssertionError(f"{what}: {len(bad)} of {g.size} pixels differ, first at {tuple(bad[0])}: "
                             f"{g[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}")


SHAPES = [((8, 12), (8, 12)), ((13, 17), (8, 12)), ((5, 7), (16, 20)), ((1, 1), (4, 4)), ((9, 33), (9, 16)),
          ((7, 9), (5, 13))]


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("src_hw, dst_hw", SHAPES, ids=[f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in SHAPES])
def test_uniform_form_equals_the_host_route(src_hw, dst_hw, mode):
    """nf of 1 and 3, random / all-255 / ramp pixels, from device and from pinned host memory; once with a row pitch of
    sw + 3 on a buffer that starts one byte past an aligned address, so that no row of any frame is aligned."""
    sh, sw = src_hw
    rng = np.random.default_rng(100 * sh + sw + mode)
    for nf in (1, 3):
        for kind in ("random", "white", "ramp"):
            src = contents(kind, rng, nf, sh, sw)
            want = host_ingest(src, dst_hw, mode)
            if src_hw == dst_hw:  # identity: the pixel itself
                assert np.array_equal(want, normalise(src, mode)[:, None])
            t = torch.from_numpy(src)
            for where, x in (("device", t.cuda()), ("pinned", t.pin_memory())):
                assert_bits(data.ingest_u8(x, dst_hw, mode), want, f"nf {nf} {kind} {where}")
    src = contents("random", rng, 3, sh, sw)
    want = host_ingest(src, dst_hw, mode)
    flat = torch.zeros(1 + 3 * sh * (sw + 3), dtype=torch.uint8)
    view = flat[1:].view(3, sh, sw + 3)[:, :, :sw]
    view.copy_(torch.from_numpy(src))
    for where, x in (("device", flat.cuda()), ("pinned", flat.pin_memory())):
        v = x[1:].view(3, sh, sw + 3)[:, None, :, :sw]  # (the (k, 1, Hs, Ws) form)
        assert v.data_ptr() % 16 == 1
        assert_bits(data.ingest_u8(v, dst_hw, mode), want, f"pitch sw + 3, {where}")


def test_pageable_source_and_out_argument():
    """A pageable host source goes through the pinned slot; out= is written in place and returned."""
    rng = np.random.default_rng(5)
    src = contents("random", rng, 2, 11, 19)
    out = torch.full((2, 1, 6, 10), float("nan"), device="cuda")
    got = data.ingest_u8(torch.from_numpy(src), (6, 10), 2, out=out)
    assert got is out
    assert_bits(out, host_ingest(src, (6, 10), 2), "pageable")
    # a second, larger source reuses the object behind ingest_u8 (the slot grows)
    src = contents("ramp", rng, 3, 20, 31)
    assert_bits(data.ingest_u8(torch.from_numpy(src), (6, 10), 0), host_ingest(src, (6, 10), 0), "pageable, grown")
    with pytest.raises(ValueError, match="out must be"):
        data.ingest_u8(torch.from_numpy(src), (6, 10), 0, out=out)


def _table_launch(rows, dh, dw, mode, dst):
    L = nat.lib()
    table = np.array(rows, dtype=np.int64).reshape(-1, 4)
    dev_table = torch.zeros(L.vad_ingest_table_bytes(len(rows)) // 8, dtype=torch.int64, device="cuda")
    nat.check(L.vad_ingest_u8_table(table.ctypes.data, len(rows), dh, dw, mode, dst.data_ptr(), dev_table.data_ptr(),
                                    nat.stream_of(dst.device)))
    torch.cuda.synchronize()  # (the pageable host table and dev_table live until here)


def test_every_size_pair_up_to_40_through_the_table_form():
    """One random sn x sn frame resized to dn x dn for every sn, dn in 1..40 -- 1,600 resizes, the 40 source sizes of
    one dn per table-form launch.  The tables' (d + 0.5) * scale - 0.5 is where a contracted fma would differ from
    the host in some of these pairs; a handful of sizes would not find it."""
    rng = np.random.default_rng(40)
    srcs = [rng.integers(0, 256, (1, sn, sn), dtype=np.uint8) for sn in range(1, 41)]
    offs = np.cumsum([0] + [s.size for s in srcs])
    flat = torch.from_numpy(np.concatenate([s.ravel() for s in srcs])).cuda()
    base = flat.data_ptr()
    rows = [(base + int(offs[i]), i + 1, i + 1, i + 1) for i in range(40)]
    bad = []
    for dn in range(1, 41):
        dst = torch.full((40, 1, dn, dn), float("nan"), device="cuda")
        _table_launch(rows, dn, dn, 1, dst)
        got = dst.cpu().numpy()
        for i, s in enumerate(srcs):
            if not np.array_equal(got[i:i + 1], host_ingest(s, (dn, dn), 1)):
                bad.append((i + 1, dn))
    assert not bad, f"{len(bad)} of 1600 (sn, dn) pairs differ from the host routine: {bad[:20]}"


@pytest.mark.parametrize("mode, dst_hw", [(0, (6, 10)), (2, (5, 13)), (1, (8, 8))])
def test_table_form_mixed_sizes_padding_and_guard(mode, dst_hw):
    """Five frames of three source sizes (one of them in pinned host memory, one with a pitch) and two padding entries
    between them: padding frames are all 0.0f, the others equal the uniform form's output and the host route, and a
    guard region behind the seven frames, prefilled with NaN like the frames, stays NaN."""
    rng = np.random.default_rng(7 + mode)
    dh, dw = dst_hw
    a = torch.from_numpy(contents("random", rng, 2, 9, 14)).cuda()
    b = torch.from_numpy(contents("random", rng, 2, 4, 5)).pin_memory()
    cbuf = torch.from_numpy(contents("random", rng, 1, 12, 7 + 3)).cuda()
    c = cbuf[:, :, :7]
    pb = nat.host_device_ptr(b)
    rows = [(a.data_ptr(), 9, 14, 14), (0, 0, 0, 0), (pb, 4, 5, 5), (pb + 20, 4, 5, 5), (0, -1, -1, -1),
            (c.data_ptr(), 12, 7, 10), (a.data_ptr() + 9 * 14, 9, 14, 14)]
    n = dh * dw
    dst = torch.full((9 * n,), float("nan"), device="cuda")
    _table_launch(rows, dh, dw, mode, dst)
    got = dst[:7 * n].view(7, 1, dh, dw)
    assert torch.isnan(dst[7 * n:]).all(), "the guard behind the nf frames was written"
    for f in (1, 4):
        assert torch.equal(got[f], torch.zeros(1, dh, dw, device="cuda")), f"padding frame {f}"
    for f, x in ((0, a[0:1]), (2, b[0:1]), (3, b[1:2]), (5, c), (6, a[1:2])):
        uni = data.ingest_u8(x, dst_hw, mode)
        assert torch.equal(got[f:f + 1], uni), f"frame {f} differs from the uniform form"
        assert_bits(got[f:f + 1], host_ingest(x.cpu().numpy(), dst_hw, mode), f"frame {f}")


def _same(a, b, what):
    if isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{what}[{i}]")
    else:
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), what


def _same_dicts(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        _same(a[k], b[k], f"{what}: {k}")


def _camera(seed, n, hs, ws):
    return np.random.default_rng(seed).integers(0, 256, (n, hs, ws), dtype=np.uint8)


PUSHES = [2, 1, 2, 2, 1, 2]  # six pushes on a ring of T + max_push - 1 = 5 slots: it wraps


@pytest.mark.parametrize("frame_size, src_hw", [((32, 48), (45, 70)), (None, (32, 48))], ids=["resize", "identity"])
def test_cad_stream_push_u8_is_push_on_host_built_frames(frame_size, src_hw):
    m = make_cad_model(dict(name="ingest", seed=3, forced=None)).cuda().eval()
    u8 = _camera(1, sum(PUSHES), *src_hw)
    x = torch.from_numpy(host_ingest(u8, frame_size or src_hw, 0)).cuda()
    kw = dict(window=4, stride=1, max_push=2, seed=5, clip0=1)
    ref, s = m.open_stream(**kw), m.open_stream(frame_size=frame_size, **kw)
    f, windows = 0, 0
    for i, k in enumerate(PUSHES):
        want = ref.push(x[f:f + k])
        src = torch.from_numpy(u8[f:f + k])
        got = s.push_u8((src.pin_memory(), src.cuda(), src)[i % 3])  # pinned, device, pageable in turn
        _same_dicts(got, want, f"push {i}")
        windows += got["anomaly_scores"].shape[0]
        f += k
    assert s.frame_size == (frame_size or src_hw) and s.frames_seen == f and windows == f - 3
    with pytest.raises(ValueError, match="max_push"):
        s.push_u8(torch.zeros(3, *src_hw, dtype=torch.uint8))


def test_ae_stream_push_u8_is_push_on_host_built_frames():
    m = make_ae_model(46).cuda().eval()
    u8 = _camera(2, sum(PUSHES), 50, 90)
    x = torch.from_numpy(host_ingest(u8, (64, 64), 2)).cuda()
    kw = dict(window=4, stride=1, max_push=2, return_reconstructions=True)
    ref, s = m.open_stream(**kw), m.open_stream(**kw)
    f = 0
    for i, k in enumerate(PUSHES):
        want = ref.push(x[f:f + k])
        src = torch.from_numpy(u8[f:f + k])
        _same_dicts(s.push_u8((src.pin_memory(), src.cuda(), src)[i % 3]), want, f"push {i}")
        f += k
    assert s.frames_seen == f and s.windows_emitted == f - 3


CAMERAS = [(40, 60), (32, 48), (57, 33)]
GROUP_KS = [(2, None, 1), (1, 2, 0), (None, 2, 2), (2, 2, 2), (0, 1, None), (1, None, 2)]


def _group_pushes(g_u8, g_ref, cams, size, mode):
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
            u8s.append((src.pin_memory(), src.cuda(), src)[(p + s) % 3] if k else src[:, None])
            xs.append(torch.from_numpy(host_ingest(chunk, size, mode)).cuda() if k
                      else torch.zeros(0, 1, *size, device="cuda"))
            seen[s] += k
        got, want = g_u8.push_u8(u8s), g_ref.push(xs)
        assert len(got) == len(want) == 3
        for s in range(3):
            _same_dicts(got[s], want[s], f"push {p} stream {s}")
    assert g_u8.frames_seen == g_ref.frames_seen == seen


def test_cad_group_push_u8_is_push_on_host_built_frames():
    """Three cameras of three source sizes; ks include None, 0 and max_push; F = 3 is padded to 4 frames, F = 6 fills
    the largest plan, F = 1 and 4 need no padding."""
    m = make_cad_model(dict(name="ingest_g", seed=4, forced=None)).cuda().eval()
    cams = [_camera(10 + s, 8, *hw) for s, hw in enumerate(CAMERAS)]
    kw = dict(window=4, stride=1, max_push=2, seed=2, clip0=[0, 5, 9], frame_size=(32, 48))
    _group_pushes(m.open_stream_group(3, **kw), m.open_stream_group(3, **kw), cams, (32, 48), 0)


def test_ae_group_push_u8_is_push_on_host_built_frames():
    m = make_ae_model(46).cuda().eval()
    cams = [_camera(20 + s, 8, *hw) for s, hw in enumerate(CAMERAS)]
    kw = dict(window=4, stride=1, max_push=2, return_reconstructions=True)
    _group_pushes(m.open_stream_group(3, **kw), m.open_stream_group(3, **kw), cams, (64, 64), 2)


def test_push_u8_leaves_other_work_on_the_engine_undisturbed():
    """A push_u8 between a clip forward and a score_video call: both return what an undisturbed run returns."""
    H, W = 32, 48
    m = make_cad_model(dict(name="ingest_iso", seed=2, forced=None)).cuda().eval()
    clip = co.synth_clips(5, 0, 0, 2, 1, H, W).cuda()  # (2, 1, 1, H, W): the plan a push of two frames borrows
    video = co.synth_clips(3, 0, 0, 1, 7, H, W)[0].cuda()
    u8 = torch.from_numpy(_camera(3, 4, 41, 53))

    def run(disturb):
        s = m.open_stream(window=2, max_push=2, seed=6, frame_size=(H, W))
        with torch.no_grad():
            a = m(clip, seed=4)
        a = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in a.items()}
        if disturb:
            s.push_u8(u8[:2].pin_memory())
            s.push_u8(u8[2:].cuda())
        return a, m.score_video(video, window=4, stride=1, chunk=2, seed=1)

    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    quiet_a, quiet_b = run(False)
    got_a, got_b = run(True)
    _same_dicts(got_a, quiet_a, "clip forward")
    _same_dicts(got_b, quiet_b, "score_video")
    for k, v in m.state_dict().items():
        assert torch.equal(v, state[k]), f"{k} changed"
