"""open_stream_group on the three clip models (a2, minicausal, bbox) without a device: every ValueError, raised before
any device work on a CPU model, the ring and plan sizes, and the (base, first) table rows of a hand-worked schedule."""
import pytest
import torch

from vad_amd import clip_stream_group as csg


def _a2():
    from vad_amd.a2 import CausalAnomalyDetector
    return CausalAnomalyDetector()


def _mc(C=1):
    from vad_amd.mc import SimpleVideoAnomalyDetector
    return SimpleVideoAnomalyDetector(input_channels=C, temporal_frames=4)


def _bbox():
    from vad_amd.bbox import CausalAnomalyDetector
    return CausalAnomalyDetector(num_frames=4)


MODELS = {"a2": (_a2, 3), "mc1": (_mc, 1), "mc3": (lambda: _mc(3), 3), "bbox": (_bbox, 3)}


@pytest.fixture(scope="module", params=list(MODELS))
def model(request):
    torch.manual_seed(0)
    make, C = MODELS[request.param]
    return make().eval(), C


def test_table_rows_of_a_hand_worked_schedule():
    """Two cameras, window 4, stride 1, max_push 2: cap 5, camera 1's ring starts at slot 5.  Camera 0 has taken 7
    frames and emitted 4 windows; camera 1 has taken 3 and emitted none.  Each brings 2 frames: camera 0's frames 7, 8
    go to slots 7 mod 5 = 2 and 3 and complete windows 4 and 5, which start at frames 4 and 5 = slots 4 and 0 of its
    ring; camera 1's frames 3, 4 go to slots 5 + 3 and 5 + 4 and complete windows 0 and 1, starting at slots 0 and 1."""
    dst, rows = csg.window_rows([7, 3], [4, 0], [2, 2], 4, 1, 5)
    assert dst == [2, 3, 8, 9]
    assert rows == [(0, 4), (0, 0), (5, 0), (5, 1)]
    # stride 3: camera 0 (8 frames; the windows at frames 0 and 3 emitted) completes the one at frame 6 = slot 1 with
    # frame 9; camera 1's third frame completes nothing
    dst, rows = csg.window_rows([8, 2], [2, 0], [2, 1], 4, 3, 5)
    assert dst == [3, 4, 7]
    assert rows == [(0, 1)]
    # a camera that brings nothing has no row, and the rows stay in camera order
    dst, rows = csg.window_rows([4, 9], [1, 6], [0, 1], 4, 1, 5)
    assert dst == [5 + 4] and rows == [(5, 1)]


def test_sizes_counters_and_reset(model):
    m, C = model
    g = m.open_stream_group(3, window=4, stride=2, max_push=3)
    assert (g.cap, g.total_slots, g.max_frames, g.max_windows, g.channels) == (6, 18, 9, 6, C)
    assert m.open_stream_group(5, window=4, stride=1, max_push=2).max_windows == 10
    g.frames_seen, g.windows_emitted = [30, 31, 32], [15, 16, 17]
    g.reset(1)
    assert g.frames_seen == [30, 0, 32] and g.windows_emitted == [15, 0, 17]
    g.reset()
    assert g.frames_seen == [0, 0, 0] and g.windows_emitted == [0, 0, 0]


def test_default_windows():
    assert _a2().eval().open_stream_group(2).window == 8
    assert _mc().eval().open_stream_group(2).window == 4       # temporal_frames
    assert _bbox().eval().open_stream_group(2).window == 4     # num_frames


@pytest.mark.parametrize("kw, text", [
    (dict(num_streams=0), "num_streams"),
    (dict(num_streams=2.5), "num_streams"),
    (dict(num_streams=2, window=4, stride=0), "stride"),
    (dict(num_streams=2, window=4, max_push=1.5), "max_push"),
    (dict(num_streams=2, window=4, frame_size=(16,)), "frame_size"),
    (dict(num_streams=2, window=4, frame_size=(1, 64)), "frame_size of at least"),
])
def test_open_stream_group_rejects_bad_arguments(model, kw, text):
    with pytest.raises(ValueError, match=text):
        model[0].open_stream_group(**kw)


@pytest.mark.parametrize("kind, least", [("a2", 1), ("mc1", 4), ("bbox", 2)])
def test_window_below_the_model_s_minimum(kind, least):
    m = MODELS[kind][0]().eval()
    with pytest.raises(ValueError, match=f"window must be an integer >= {least}"):
        m.open_stream_group(2, window=least - 1)
    m.open_stream_group(2, window=least)


def test_a_group_larger_than_the_plan_limit_names_the_limit():
    a2, mc = _a2().eval(), _mc().eval()
    with pytest.raises(ValueError, match=r"at most 256 .*A2_MAXB.* 257 \* 1 = 257"):
        a2.open_stream_group(257, window=4)
    with pytest.raises(ValueError, match=r"at most 256 .*A2_MAXB.* 65 \* 4 = 260"):
        a2.open_stream_group(65, window=4, stride=2, max_push=8)
    assert a2.open_stream_group(256, window=4).max_windows == 256
    assert a2.open_stream_group(128, window=4, stride=2, max_push=4).max_windows == 256
    with pytest.raises(ValueError, match=r"at most 1024 .*MC_MAXB.* 1025 \* 1 = 1025"):
        mc.open_stream_group(1025, window=4)
    assert mc.open_stream_group(1024, window=4).max_windows == 1024


def _f(k, c, h=16, w=16):
    return torch.zeros(k, c, h, w)


def test_push_rejects_bad_frames_without_a_device(model):
    m, C = model
    other = 1 if C == 3 else 3
    for frames, text in [
            ([_f(1, C)], "num_streams = 2"),
            ([_f(1, C)] * 3, "num_streams = 2"),
            (_f(2, C), "num_streams = 2"),
            ([_f(3, C), _f(1, C)], "max_push = 2"),
            ([_f(1, C), _f(1, C, h=24)], "frame size"),
            ([_f(1, C), _f(1, other)], f"frames of shape \\(N, {C}, H, W\\)"),
            ([_f(1, C), torch.zeros(1, 16, 16)], "stream 1: frames of shape"),
            ([_f(1, C), _f(1, C).to(torch.uint8)], "floating point"),
            ([_f(1, C, h=1, w=1), None], "frames of at least"),
            ([None, None], "no stream brought a frame"),
            ([_f(0, C), None], "no stream brought a frame")]:
        g = m.open_stream_group(2, window=4, max_push=2)
        with pytest.raises(ValueError, match=text):
            g.push(frames)
        assert g.frames_seen == [0, 0] and g.windows_emitted == [0, 0] and g.frame_size is None and g._ring is None


def test_push_rejects_a_frame_size_other_than_the_groups(model):
    m, C = model
    g = m.open_stream_group(2, window=4, max_push=2, frame_size=(16, 16))
    with pytest.raises(ValueError, match="frame size"):
        g.push([_f(1, C, h=24), None])
    kind = g.kind
    chunks, ks, size = csg.check_group_push(kind, m, [None, _f(2, C)], 2, 2, None)
    assert chunks[0] is None and chunks[1].shape == (2, C, 16, 16) and ks == [0, 2] and size == (16, 16)


def test_group_rejects_training_mode(model):
    m, C = model
    g = m.open_stream_group(2, window=4, frame_size=(16, 16))
    u8 = torch.zeros(1, 20, 20, dtype=torch.uint8) if C == 1 else torch.zeros(1, 20, 20, 3, dtype=torch.uint8)
    m.train()
    try:
        with pytest.raises(ValueError, match="eval mode"):
            m.open_stream_group(2, window=4)
        with pytest.raises(ValueError, match="eval mode"):
            g.push([_f(1, C), _f(1, C)])
        with pytest.raises(ValueError, match="eval mode"):
            g.push([None, None])
        with pytest.raises(ValueError, match="eval mode"):
            g.push_u8([u8, u8], color=None if C == 1 else "bgr")
    finally:
        m.eval()


def test_push_u8_rejects_bad_frames_without_a_device(model):
    m, C = model
    grey = torch.zeros(1, 20, 20, dtype=torch.uint8)
    bgr = torch.zeros(1, 20, 20, 3, dtype=torch.uint8)
    g = m.open_stream_group(2, window=4, max_push=2, frame_size=(16, 16))
    if C == 3:
        with pytest.raises(ValueError, match="name the frames' colour format"):
            g.push_u8([bgr, bgr])
        with pytest.raises(ValueError, match="4 bytes per pixel"):
            g.push_u8([bgr, bgr], color="bgrx")  # one format per call
    else:
        with pytest.raises(ValueError, match="stream 1"):
            g.push_u8([grey, bgr])
    good, color = (grey, None) if C == 1 else (bgr, "bgr")
    for frames, text in [([good], "num_streams = 2"), ([good.expand(3, *good.shape[1:]), good], "max_push = 2"),
                         ([None, None], "no stream brought a frame"), ([good, good.float()], "uint8")]:
        with pytest.raises(ValueError, match=text):
            g.push_u8(frames, color=color)
    with pytest.raises(ValueError, match="does not know its frame size"):
        m.open_stream_group(2, window=4).push_u8([good, good], color=color)
    with pytest.raises(ValueError, match="but the model is on cpu"):
        g.push_u8([good, good], color=color)  # every check passed: the device is asked for last
    assert g.frames_seen == [0, 0] and g._ring is None and g._ingest is None
