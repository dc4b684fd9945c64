"""ClipStream (open_stream on the a2, minicausal and bbox clip models), the parts that need no GPU: the ring size,
the windows a push sequence completes against score_video's enumeration, the slots frames go to, and every ValueError
raised before any device work."""
import pytest
import torch

from tests.test_clip_score_video import a2_model, mc_model

PUSHES = (3, 1, 2, 3, 3, 1, 1, 3)  # 17 frames


def bbox_model(T=4):
    from vad_amd.bbox import CausalAnomalyDetector
    torch.manual_seed(0)
    return CausalAnomalyDetector(num_frames=T).eval()


MODELS = {"a2": (a2_model, 3), "mc": (mc_model, 1), "bbox": (bbox_model, 3)}


@pytest.mark.parametrize("kind", list(MODELS))
def test_ring_holds_window_plus_max_push_minus_one_frames(kind):
    from vad_amd.clip_stream import ClipStream, ring_slots
    make, C = MODELS[kind]
    for window, max_push in [(4, 3), (4, 1), (8, 5)]:
        st = make().open_stream(window=window, max_push=max_push)
        assert isinstance(st, ClipStream) and st.kind == kind and st.channels == C
        assert st.cap == ring_slots(window, max_push) == window + max_push - 1
        assert st._ring is None  # allocated at the first push, on the frames' device
    assert make().open_stream(window=4, stride=3, max_push=3).max_windows == 1
    assert make().open_stream(window=4, stride=2, max_push=3).max_windows == 2
    assert make().open_stream(window=4, stride=1, max_push=3).max_windows == 3


def test_mc_and_bbox_window_default_to_the_model_s_clip_length():
    assert mc_model(T=6).open_stream().window == 6
    assert bbox_model(T=5).open_stream().window == 5
    assert a2_model().open_stream().window == 8


@pytest.mark.parametrize("stride", [1, 3])
def test_window_starts_of_a_push_sequence_are_score_video_s(stride):
    """The bookkeeping a push does (stream_util.stream_schedule, then the two counters), without the device: the
    windows of the 17 frames come out once each, in order, and every one lies inside the ring when it is scored."""
    from vad_amd.clip_stream import window_starts
    from vad_amd.stream_util import stream_schedule
    st = a2_model().open_stream(window=4, stride=stride, max_push=3)
    assert st.cap == 6
    starts, empty = [], 0
    for k in PUSHES:
        slots = st._slots(k)
        assert sum(n for _, n, _ in slots) == k and all(0 <= s0 and s0 + n <= st.cap for s0, n, _ in slots)
        assert [s0 for s0, _, _ in slots][0] == st.frames_seen % st.cap
        first, widx0, nw = stream_schedule(st.frames_seen, st.windows_emitted, k, st.window, st.stride)
        assert 0 <= nw <= st.max_windows
        total = st.frames_seen + k
        empty += nw == 0 and total >= st.window  # (before the first window is in, every push is empty)
        for i in range(nw):  # the ring holds frames total - cap .. total - 1
            s = first + i * stride
            assert total - st.cap <= s and s + st.window <= total
            starts.append(s)
        if nw:
            assert (nw - 1) * stride + st.window <= st.cap  # what the library's ring check asks of one call
        st.frames_seen, st.windows_emitted = total, widx0 + nw
    assert starts == window_starts(sum(PUSHES), 4, stride).tolist()
    assert (empty > 0) == (stride == 3)  # stride 3: some later pushes complete no window either
    st.reset()
    assert st.frames_seen == st.windows_emitted == 0


def test_slots_straddle_the_ring_s_end_in_two_runs():
    st = a2_model().open_stream(window=4, max_push=3)  # 6 slots
    st.frames_seen = 5
    assert st._slots(3) == [(5, 1, 0), (0, 2, 1)]
    st.frames_seen = 16
    assert st._slots(2) == [(4, 2, 0)]


@pytest.mark.parametrize("kind", list(MODELS))
def test_open_stream_value_errors(kind):
    make, _ = MODELS[kind]
    least = {"a2": 1, "mc": 4, "bbox": 2}[kind]
    for kw, text in [(dict(window=least - 1), f"window must be an integer >= {least}"),
                     (dict(window=4.5), "window must be an integer"),
                     (dict(window=4, stride=0), "stride must be an integer >= 1"),
                     (dict(window=4, stride=1.5), "stride must be an integer >= 1"),
                     (dict(window=4, max_push=0), "max_push must be an integer >= 1"),
                     (dict(window=4, max_push=True), "max_push must be an integer >= 1"),
                     (dict(window=4, frame_size=(10,)), "frame_size must be None or"),
                     (dict(window=4, frame_size=(1, 64)), "frame_size of at least")]:
        with pytest.raises(ValueError, match=text):
            make().open_stream(**kw)
    m = make()
    m.train()
    with pytest.raises(ValueError, match="eval mode"):
        m.open_stream(window=4)


@pytest.mark.parametrize("kind", list(MODELS))
def test_push_value_errors_come_before_any_device_work(kind):
    make, C = MODELS[kind]
    m = make()
    st = m.open_stream(window=4, stride=1, max_push=3, frame_size=(10, 13))
    ok = torch.rand(2, C, 10, 13)
    for frames, text in [(torch.rand(2, C, 10), "frames of shape"),
                         (torch.rand(2, C + 1, 10, 13), "frames of shape"),
                         ((ok * 255).to(torch.uint8), "floating point"),
                         (torch.rand(4, C, 10, 13), "between 1 and max_push = 3 frames per push, got 4"),
                         (torch.rand(0, C, 10, 13), "between 1 and max_push = 3 frames per push, got 0"),
                         (torch.rand(2, C, 10, 14), r"frames of \(10, 14\), but the stream's frames are \(10, 13\)")]:
        with pytest.raises(ValueError, match=text):
            st.push(frames)
    m.train()
    with pytest.raises(ValueError, match="eval mode"):
        st.push(ok)
    with pytest.raises(ValueError, match="eval mode"):
        st.push_u8(torch.zeros(2, 20, 31, 3, dtype=torch.uint8), color="bgr")
    m.eval()
    with pytest.raises(RuntimeError, match="HIP"):  # every check passed: the first device-dependent step refuses
        st.push(ok)
    assert st._ring is None and st.frames_seen == 0 and m._engine is None


@pytest.mark.parametrize("kind", list(MODELS))
def test_push_u8_value_errors_come_before_any_device_work(kind):
    make, C = MODELS[kind]
    st = make().open_stream(window=4, max_push=2, frame_size=(10, 13))
    grey, bgr = torch.zeros(2, 20, 31, dtype=torch.uint8), torch.zeros(2, 20, 31, 3, dtype=torch.uint8)
    if C == 3:
        with pytest.raises(ValueError, match="name the frames' colour format"):
            st.push_u8(grey)
    with pytest.raises(ValueError, match="must be uint8"):
        st.push_u8(bgr.float(), color="bgr")
    with pytest.raises(ValueError, match="between 1 and max_push = 2 frames per push, got 3"):
        st.push_u8(torch.zeros(3, 20, 31, 3, dtype=torch.uint8), color="bgr")
    with pytest.raises(ValueError, match="bytes per pixel"):
        st.push_u8(bgr, color="bgrx")
    with pytest.raises(ValueError, match="frames on cpu, but the model is on cpu"):  # host frames need a HIP model
        st.push_u8(bgr, color="bgr")
    late = make().open_stream(window=4, max_push=2)  # no frame_size, and no push has set one
    with pytest.raises(ValueError, match="pass frame_size"):
        late.push_u8(bgr, color="bgr")
    assert st._ring is None and st._ingest is None


def test_push_u8_refuses_a_model_that_reads_neither_grey_nor_rgb():
    st = mc_model(C=2).open_stream(frame_size=(10, 13))
    with pytest.raises(ValueError, match="grey or RGB frames only"):
        st.push_u8(torch.zeros(1, 20, 31, dtype=torch.uint8))
