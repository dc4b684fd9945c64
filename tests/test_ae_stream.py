"""VideoAutoEncoder.open_stream without a device: the argument checks of open_stream and push, which raise before any
device work, the ring size, the counters and reset().  (The push schedule is stream.stream_schedule, checked against a
brute-force enumeration in tests/test_stream.py.)"""
import pytest
import torch

from vad_amd import ae_stream as ast
from vad_amd import stream as st
from vad_amd.ae import VideoAutoEncoder


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return VideoAutoEncoder().eval()


@pytest.mark.parametrize("kw, text", [
    (dict(window=0), "window"),
    (dict(window=2.5), "window"),
    (dict(window=True), "window"),
    (dict(window=4, stride=0), "stride"),
    (dict(window=4, stride="2"), "stride"),
    (dict(window=4, max_push=0), "max_push"),
    (dict(window=4, max_push=1.5), "max_push"),
    (dict(window=4, max_push=501), "max_push must be at most 500"),
])
def test_open_stream_rejects_bad_arguments(model, kw, text):
    with pytest.raises(ValueError, match=text):
        model.open_stream(**kw)


def test_the_schedule_is_the_cad_stream_s():
    """Reused, not copied."""
    assert ast.stream_schedule is st.stream_schedule and ast._positive_int is st._positive_int


def test_open_stream_and_push_reject_training_mode(model):
    s = model.open_stream(window=4)
    model.train()
    try:
        with pytest.raises(ValueError, match="eval mode"):
            model.open_stream(window=4)
        with pytest.raises(ValueError, match="eval mode"):
            s.push(torch.zeros(1, 1, 64, 64))
    finally:
        model.eval()
    assert s.frames_seen == 0 and s.windows_emitted == 0


@pytest.mark.parametrize("frames, text", [
    (torch.zeros(0, 1, 64, 64), "max_push = 2 frames per push, got 0"),
    (torch.zeros(3, 1, 64, 64), "max_push = 2 frames per push, got 3"),
    (torch.zeros(1, 3, 1, 64, 64), "max_push = 2 frames per push, got 3"),
    (torch.zeros(2, 64, 64), r"\(k, 1, 64, 64\) or \(1, k, 1, 64, 64\), got \(2, 64, 64\)"),
    (torch.zeros(2, 1, 1, 64, 64), "one stream per call, got a batch of 2"),
    (torch.zeros(2, 1, 48, 64), r"64x64 single-channel frames.*got \(2, 1, 48, 64\)"),
    (torch.zeros(1, 2, 1, 48, 64), r"64x64 single-channel frames.*got \(2, 1, 48, 64\)"),
    (torch.zeros(2, 3, 64, 64), "64x64 single-channel frames"),
])
def test_push_rejects_bad_frames_without_a_device(model, frames, text):
    s = model.open_stream(window=4, max_push=2)
    with pytest.raises(ValueError, match=text):
        s.push(frames)
    assert s.frames_seen == 0 and s.windows_emitted == 0 and s._ring is None


@pytest.mark.parametrize("frames", [torch.zeros(2, 1, 64, 64), torch.zeros(1, 3, 1, 64, 64), torch.zeros(1, 1, 64, 64)])
def test_legal_arguments_reach_the_device_check(model, frames):
    """Every argument legal on a CPU model: the first thing to fail is the device requirement, not a ValueError."""
    s = model.open_stream(window=4, stride=2, max_push=3, return_reconstructions=True)
    with pytest.raises(RuntimeError, match="HIP"):
        s.push(frames)
    assert s.frames_seen == 0 and s.windows_emitted == 0
    assert ast.check_push(model, frames, 3).shape == (frames.shape[-4], 1, 64, 64)


def test_stream_counters_and_ring_size(model):
    s = model.open_stream(window=16, max_push=8)
    assert (s.cap, s.frames_seen, s.windows_emitted) == (23, 0, 0)
    assert (s.window, s.stride, s.max_push, s.return_reconstructions) == (16, 1, 8, False)
    assert model.open_stream().cap == 16 and model.open_stream(window=4, stride=3, max_push=500).cap == 503
    s.frames_seen, s.windows_emitted = 30, 15
    s.reset()
    assert (s.frames_seen, s.windows_emitted) == (0, 0)
