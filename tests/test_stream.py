"""CausalAnomalyDetector.open_stream without a device: the push schedule against a brute-force enumeration on a
simulated ring, and the argument checks, which raise before any device work."""
import random

import pytest
import torch

from vad_amd import stream as st
from vad_amd.cad import CausalAnomalyDetector


@pytest.mark.parametrize("window", [1, 4, 5])
@pytest.mark.parametrize("stride", [1, 2, 3, 7])
@pytest.mark.parametrize("max_push", [1, 2, 3, 8])
def test_schedule_against_brute_force(window, stride, max_push):
    """Pushes of random sizes 1..max_push up to 40 frames, on a ring of cap = window + max_push - 1 slots that
    records which frame each slot holds: every window is emitted exactly once, in order, by the push that brings its
    last frame; a batch has at most k windows and spans at most cap frames; every frame a batch reads is still in
    its slot."""
    cap = window + max_push - 1
    rng = random.Random(1000 * window + 10 * stride + max_push)
    ring = [None] * cap
    seen = emitted = 0
    got = []
    while seen < 40:
        k = rng.randint(1, max_push)
        for g in range(seen, seen + k):
            ring[g % cap] = g
        first, widx0, nw = st.stream_schedule(seen, emitted, k, window, stride)
        # brute force: the windows whose last frame is among the k new ones
        want = [w for w in range(seen + k) if seen <= w * stride + window - 1 < seen + k]
        assert list(range(widx0, widx0 + nw)) == want
        assert 0 <= nw <= k
        if nw:
            assert first == widx0 * stride
            assert (nw - 1) * stride + window <= cap
            for i in range(nw):
                for t in range(window):
                    g = first + i * stride + t
                    assert ring[g % cap] == g, f"frame {g} of window {widx0 + i} was overwritten"
        got += want
        seen += k
        emitted += nw
    assert got == list(range((seen - window) // stride + 1))


def test_schedule_of_a_whole_video_in_one_push():
    assert st.stream_schedule(0, 0, 8, 4, 1) == (0, 0, 5)
    assert st.stream_schedule(0, 0, 3, 4, 1) == (0, 0, 0)
    assert st.stream_schedule(3, 0, 1, 4, 1) == (0, 0, 1)
    # stride > window: windows 0-1, 5-6, 10-11; frames 2-4 and 7-9 fill no window
    assert st.stream_schedule(3, 1, 3, 2, 5) == (5, 1, 0)
    assert st.stream_schedule(9, 2, 3, 2, 5) == (10, 2, 1)


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return CausalAnomalyDetector().eval()


@pytest.mark.parametrize("kw, text", [
    (dict(window=0), "window"),
    (dict(window=2.5), "window"),
    (dict(window=4, stride=0), "stride"),
    (dict(window=4, stride="2"), "stride"),
    (dict(window=4, max_push=0), "max_push"),
    (dict(window=4, max_push=1.5), "max_push"),
])
def test_open_stream_rejects_bad_arguments(model, kw, text):
    with pytest.raises(ValueError, match=text):
        model.open_stream(**kw)


def test_open_stream_and_push_reject_training_mode_and_bf16(model):
    s = model.open_stream(window=4)
    x = torch.zeros(1, 1, 32, 32)
    model.train()
    try:
        with pytest.raises(ValueError, match="eval mode"):
            model.open_stream(window=4)
        with pytest.raises(ValueError, match="eval mode"):
            s.push(x)
    finally:
        model.eval()
    model.set_compute_dtype(torch.bfloat16)
    try:
        with pytest.raises(ValueError, match="fp32 only"):
            model.open_stream(window=4)
        with pytest.raises(ValueError, match="fp32 only"):
            s.push(x)
    finally:
        model.set_compute_dtype(torch.float32)


@pytest.mark.parametrize("frames, text", [
    (torch.zeros(3, 1, 32, 32), "max_push"),
    (torch.zeros(0, 1, 32, 32), "max_push"),
    (torch.zeros(1, 3, 1, 32, 32), "max_push"),
    (torch.zeros(2, 3, 32, 32), "single-channel"),
    (torch.zeros(2, 32, 32), "shape"),
    (torch.zeros(2, 1, 1, 32, 32), "one stream per call"),
])
def test_push_rejects_bad_frames_without_a_device(model, frames, text):
    s = model.open_stream(window=4, max_push=2)
    with pytest.raises(ValueError, match=text):
        s.push(frames)
    assert s.frames_seen == 0 and s.windows_emitted == 0 and s.frame_size is None


def test_push_rejects_a_frame_size_other_than_the_first(model):
    # (the first push needs a device; its effect on the check is the recorded frame size)
    with pytest.raises(ValueError, match="frame size"):
        st.check_push(model, torch.zeros(1, 1, 32, 48), 2, (32, 32))
    assert st.check_push(model, torch.zeros(1, 2, 1, 32, 32), 2, (32, 32)).shape == (2, 1, 32, 32)
    assert st.check_push(model, torch.zeros(1, 1, 32, 48), 2, None).shape == (1, 1, 32, 48)


def test_stream_counters_and_ring_size(model):
    s = model.open_stream(window=16, max_push=8)
    assert (s.cap, s.frames_seen, s.windows_emitted) == (23, 0, 0)
    s.frames_seen, s.windows_emitted = 30, 15
    s.reset()
    assert (s.frames_seen, s.windows_emitted) == (0, 0)
