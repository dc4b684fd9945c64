"""VideoAutoEncoder.open_stream_group without a device: the argument checks of open_stream_group and push, which raise
before the library or a device is touched, the plan-size rule, the ring sizes, the counters and reset().  (The push
tables are stream_group.group_schedule, checked against a brute-force enumeration in tests/test_stream_group.py.)"""
import pytest
import torch

from vad_amd import ae_stream_group as asg
from vad_amd import stream as st
from vad_amd import stream_group as sg
from vad_amd.ae import VideoAutoEncoder


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return VideoAutoEncoder().eval()


@pytest.fixture
def no_library(monkeypatch):
    """Any use of the library fails the test: the checks under test come before it."""
    def lib():
        raise AssertionError("the library was touched before the argument check")
    monkeypatch.setattr(asg.nat, "lib", lib)


@pytest.mark.parametrize("kw, text", [
    (dict(num_streams=0), "num_streams"),
    (dict(num_streams=2.5), "num_streams"),
    (dict(num_streams=2, window=0), "window"),
    (dict(num_streams=2, window=True), "window"),
    (dict(num_streams=2, stride=0), "stride"),
    (dict(num_streams=2, stride="2"), "stride"),
    (dict(num_streams=2, max_push=0), "max_push"),
    (dict(num_streams=2, max_push=1.5), "max_push"),
    (dict(num_streams=501), "num_streams \\* max_push must be at most 500"),
    (dict(num_streams=167, max_push=3), "167 \\* 3 = 501"),
])
def test_open_stream_group_rejects_bad_arguments(model, no_library, kw, text):
    with pytest.raises(ValueError, match=text):
        model.open_stream_group(**kw)


def test_the_schedule_and_the_padding_are_the_cad_groups(model):
    """Reused, not copied."""
    assert asg.group_schedule is sg.group_schedule and asg.padded_frames is sg.padded_frames
    assert asg.stream_schedule is st.stream_schedule and asg._positive_int is st._positive_int


def test_a_plan_of_500_frames_is_accepted_and_501_refused(model, no_library):
    """A plan holds at most model.memory_size = 500 clips (vad_ae_create), so that is the largest push."""
    assert model.memory_size == 500
    for S, K in [(500, 1), (1, 500), (125, 4), (20, 25)]:
        g = model.open_stream_group(S, window=4, max_push=K)
        assert g.max_frames == 500 and g.cap == 4 + K - 1 and g.total_slots == S * g.cap
    for S, K in [(501, 1), (1, 501), (167, 3), (3, 167)]:
        with pytest.raises(ValueError, match="must be at most 500"):
            model.open_stream_group(S, window=4, max_push=K)


@pytest.mark.parametrize("limit", [1, 3, 12, 96, 500])
def test_padded_sizes_never_exceed_the_cap(limit):
    sizes = {sg.padded_frames(f, limit) for f in range(1, limit + 1)}
    assert max(sizes) == limit and len(sizes) <= (limit - 1).bit_length() + 1
    for f in range(1, limit + 1):
        p = sg.padded_frames(f, limit)
        assert f <= p <= limit and (p == limit or p & (p - 1) == 0)


def _f(k, c=1, h=64, w=64):
    return torch.zeros(k, c, h, w)


@pytest.mark.parametrize("frames, text", [
    ([_f(1)], "num_streams = 2 entries"),
    ([_f(1), _f(1), _f(1)], "num_streams = 2 entries.*got 3 entries"),
    (_f(2), "num_streams = 2 entries.*got Tensor"),
    ([_f(3), _f(1)], "stream 0: at most max_push = 2 frames per push, got 3"),
    ([_f(1), _f(1, h=48)], r"stream 1: frames of shape \(k, 1, 64, 64\) or None.*got \(1, 1, 48, 64\)"),
    ([_f(1), _f(1, c=3)], r"stream 1: frames of shape \(k, 1, 64, 64\)"),
    ([_f(1), torch.zeros(1, 64, 64)], r"stream 1: frames of shape \(k, 1, 64, 64\)"),
    ([_f(1), torch.zeros(1, 1, 1, 64, 64)], r"stream 1: frames of shape \(k, 1, 64, 64\)"),
    ([_f(1), 3], r"stream 1: frames of shape \(k, 1, 64, 64\)"),
    ([None, None], "no stream brought a frame"),
    ([_f(0), None], "no stream brought a frame"),
])
def test_push_rejects_bad_frames_without_a_device(model, no_library, frames, text):
    g = model.open_stream_group(2, window=4, max_push=2)
    with pytest.raises(ValueError, match=text):
        g.push(frames)
    assert g.frames_seen == [0, 0] and g.windows_emitted == [0, 0] and g._ring is None


def test_group_rejects_training_mode(model, no_library):
    g = model.open_stream_group(2, window=4)
    model.train()
    try:
        with pytest.raises(ValueError, match="eval mode"):
            model.open_stream_group(2, window=4)
        with pytest.raises(ValueError, match="eval mode"):
            g.push([_f(1), _f(1)])
    finally:
        model.eval()
    assert g.frames_seen == [0, 0] and g.windows_emitted == [0, 0]


def test_legal_arguments_reach_the_device_check(model):
    """Every argument legal on a CPU model: the first thing to fail is the device requirement, not a ValueError."""
    g = model.open_stream_group(3, window=4, stride=2, max_push=3, return_reconstructions=True)
    with pytest.raises(RuntimeError, match="HIP"):
        g.push((_f(2), None, _f(0)))
    assert g.frames_seen == [0, 0, 0] and g.windows_emitted == [0, 0, 0]
    chunks, ks = asg.check_group_push(model, [None, _f(2), _f(0)], 3, 2)
    assert chunks[0] is None and chunks[1].shape == (2, 1, 64, 64) and chunks[2] is None and ks == [0, 2, 0]


def test_group_counters_ring_sizes_and_reset(model):
    g = model.open_stream_group(3, window=16, max_push=8)
    assert (g.cap, g.total_slots, g.max_frames) == (23, 69, 24)
    assert (g.num_streams, g.window, g.stride, g.max_push, g.return_reconstructions) == (3, 16, 1, 8, False)
    assert model.open_stream_group(4).cap == 16
    g.frames_seen, g.windows_emitted = [30, 31, 32], [15, 16, 17]
    g.reset(1)
    assert g.frames_seen == [30, 0, 32] and g.windows_emitted == [15, 0, 17]
    g.reset()
    assert g.frames_seen == [0, 0, 0] and g.windows_emitted == [0, 0, 0]
