"""ClipStream on the GPU, for the a2, minicausal (grey and 3-channel) and bbox clip models: a push scores the windows it
completes straight from the ring of raw frames, and must give bit for bit what ``model(clips)`` gives for those windows
gathered with torch into one batch (a2, one window: the clip twice, row 0) -- the windows call runs the clip path's
kernels on the same number of clips, only the first layer's load addresses differ.

window 4 and max_push 3 make a ring of 6 slots; 17 frames pushed as 3, 1, 2, 3, 3, 1, 1, 3 start a push at every slot
of the ring, and windows straddle its end with their first, middle and last frame.  With stride 3 some pushes complete
no window: they return empty tensors and queue nothing.

Against score_video, which batches the windows differently.  The clip path is not blind to the batch: bbox's head
GEMMs (dense_fwd) pick their kernel by the number of rows -- up to 8, up to 16, more -- and within one kernel a row's
arithmetic does not depend on the others; a2's conv3d_2 / conv3d_3 GEMMs split their reduction by the number of output
tiles, at most cdiv(K, 128) ways (4 and 7), and at 10 x 13 frames and T = 4 a clip has 24 and 4 output rows, so any
batch of up to 14 clips is a handful of tiles, far below the 512 / 7 at which the split would shrink; minicausal has no
such choice.  A push here completes at most 3 windows, so score_video is asked for batches of 8: both sides then run
the same kernels with the same split, and the concatenated pushes must equal it bit for bit."""
import pytest
import torch

from tests.test_clip_score_video_gpu import CHANNELS, KEYS, KINDS, assert_same, clip_call, gather, make, video
from vad_amd import data

pytestmark = pytest.mark.gpu

PUSHES = (3, 1, 2, 3, 3, 1, 1, 3)  # 17 frames
H, W = 10, 13


def run_stream(st, x, pushes=PUSHES):
    outs, f = [], 0
    for k in pushes:
        outs.append(st.push(x[f:f + k]))
        f += k
    return outs


def concat(kind, outs):
    o = {k: torch.cat([p[k] for p in outs]) for k in KEYS[kind]}
    o["window_starts"] = torch.cat([p["window_starts"] for p in outs])
    return o


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_pushes_are_the_clip_path_and_score_video(kind, stride):
    m = make(kind)
    x = video(40 + stride, sum(PUSHES), CHANNELS[kind], H, W)
    st = m.open_stream(window=4, stride=stride, max_push=3)
    assert st.cap == 6
    launches = 0
    outs, f = [], 0
    for k in PUSHES:
        o = st.push(x[f:f + k])
        f += k
        starts = o["window_starts"].tolist()
        assert o["window_starts"].dtype == torch.int64
        assert starts == [s for s in range(0, f - 3, stride) if s + 4 > f - k]  # the windows these k frames complete
        if starts:
            assert_same(kind, o, clip_call(kind, m, gather(x, 4, starts)), f"push ending at frame {f}")
            launches += 1
        else:
            assert all(o[key].shape[0] == 0 for key in KEYS[kind])
        outs.append(o)
    assert launches < len(PUSHES) if stride == 3 else launches == len(PUSHES) - 1
    assert st.frames_seen == 17 and st._ring.shape == (6, CHANNELS[kind], H, W)
    got = concat(kind, outs)
    want = m.score_video(x, window=4, stride=stride, batch=8)  # (the module docstring: why 8)
    assert got["window_starts"].tolist() == want["window_starts"].tolist() == list(range(0, 14, stride))
    assert_same(kind, got, tuple(want[k] for k in KEYS[kind]), "score_video")
    assert got["anomaly_scores"].unique().numel() > 1


@pytest.mark.parametrize("kind", KINDS)
def test_empty_pushes_queue_nothing(kind):
    """A push that completes no window copies its frames and returns empty tensors: the library is not called (a call
    with nw = 0 would be refused), and the next push scores from the right slots."""
    m = make(kind)
    x = video(43, 9, CHANNELS[kind], H, W)
    st = m.open_stream(window=4, stride=3, max_push=3)
    st.push(x[0:3])
    eng = m.scoring_engine(x.device)
    calls = []
    real = eng.windows_forward
    eng.windows_forward = lambda *a, **kw: (calls.append(a[4]), real(*a, **kw))[1]
    try:
        a = st.push(x[3:4])    # frames 0..3: window 0
        b = st.push(x[4:6])    # frames 4, 5: nothing (window 3 needs frame 6)
        c = st.push(x[6:9])    # window 3
    finally:
        del eng.windows_forward
    assert calls == [1, 1]
    assert a["window_starts"].tolist() == [0] and b["window_starts"].tolist() == [] and c["window_starts"].tolist() == [3]
    assert all(b[k].shape[0] == 0 and b[k].is_cuda for k in KEYS[kind])
    assert_same(kind, c, clip_call(kind, m, gather(x, 4, [3])))


@pytest.mark.parametrize("kind", KINDS)
def test_two_streams_on_one_model_do_not_disturb_each_other(kind):
    m = make(kind)
    C = CHANNELS[kind]
    xa, xb = video(44, 17, C, H, W), video(45, 17, C, H, W)
    alone = concat(kind, run_stream(m.open_stream(window=4, stride=1, max_push=3), xa))
    sa, sb = m.open_stream(window=4, stride=1, max_push=3), m.open_stream(window=4, stride=1, max_push=3)
    outs, f = [], 0
    for k in PUSHES:
        outs.append(sa.push(xa[f:f + k]))
        sb.push(xb[f:f + k])
        f += k
    assert sa._ring.data_ptr() != sb._ring.data_ptr()
    assert_same(kind, concat(kind, outs), tuple(alone[k] for k in KEYS[kind]))


@pytest.mark.parametrize("kind", KINDS)
def test_stream_at_64x64_with_the_model_s_default_window(kind):
    m = make(kind, T=4)
    T = 8 if kind == "a2" else 4
    x = video(46, T + 4, CHANNELS[kind], 64, 64)
    st = m.open_stream(stride=2, max_push=2) if kind != "a2" else m.open_stream(window=8, stride=2, max_push=2)
    assert st.window == T and st.cap == T + 1
    f = 0
    for k in (2,) * (T // 2 + 2):
        o = st.push(x[f:f + k])
        f += k
        starts = o["window_starts"].tolist()
        assert starts == ([f - T] if f >= T else [])
        if starts:
            assert_same(kind, o, clip_call(kind, m, gather(x, T, starts)))


def camera(seed, k, Hs, Ws, C):
    shape = (k, Hs, Ws) if C == 1 else (k, Hs, Ws, 3)
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("size, src", [((10, 13), (20, 31)), ((64, 64), (40, 50))],
                         ids=["10x13-through-the-buffer", "64x64-into-the-slots"])
@pytest.mark.parametrize("kind", ["mc1", "a2", "bbox"])
def test_push_u8_is_push_of_ingest_u8(kind, size, src):
    """u8 sources of another size than the model's frames: grey for the 1-channel minicausal, packed BGR for a2 and
    bbox.  Pushes of 3, 2, 3, 1: the third starts at slot 5 of 6 and straddles the ring's end.  A slot of 10 x 13
    frames is not 16-byte aligned for odd slots, so those go through the stream's buffer; 64 x 64 slots take the
    ingest's stores directly, in two launches across the end."""
    C = CHANNELS[kind]
    color = None if C == 1 else "bgr"
    m = make(kind)
    u8 = camera(47, 9, *src, C)
    a = m.open_stream(window=4, stride=1, max_push=3, frame_size=size)
    b = m.open_stream(window=4, stride=1, max_push=3, frame_size=size)
    assert (a._slots(1), (C * size[0] * size[1]) % 4 == 0) == ([(0, 1, 0)], size == (64, 64))
    f = 0
    for i, k in enumerate((3, 2, 3, 1)):
        chunk = u8[f:f + k]
        if i == 2:
            assert len(a._slots(k)) == 2
        if i % 2:
            chunk = chunk.cuda()  # a device source and a pageable host source in turn
        got = a.push_u8(chunk, color=color)
        want = b.push(data.ingest_u8(u8[f:f + k].cuda(), size, 1, color=color, planes=C))
        f += k
        assert got["window_starts"].tolist() == want["window_starts"].tolist()
        assert_same(kind, got, tuple(want[key] for key in KEYS[kind]), f"push {i}")
        assert torch.equal(a._ring, b._ring)
    assert got["window_starts"].tolist() == [5]
    assert (a._u8 is None) == (size == (64, 64))


def test_push_u8_luma_for_a_grey_model_and_first_push_sets_the_frame_size():
    m = make("mc1")
    u8 = camera(48, 5, 20, 31, 3)
    a = m.open_stream(window=4, max_push=3)
    first = data.ingest_u8(u8[:3].cuda(), (H, W), 1, color="rgb")
    a.push(first)  # an fp32 push fixes the stream's frame size
    assert a.frame_size == (H, W)
    got = a.push_u8(u8[3:5], color="rgb")
    b = m.open_stream(window=4, max_push=3)
    b.push(first)
    want = b.push(data.ingest_u8(u8[3:5].cuda(), (H, W), 1, color="rgb"))
    assert got["window_starts"].tolist() == [0, 1]
    assert_same("mc1", got, (want["anomaly_scores"],))
    with pytest.raises(ValueError, match="but the stream's frames are"):
        a.push(torch.rand(1, 1, 12, 13).cuda())
