"""CausalAnomalyDetector.open_stream_group without a device: the push tables against a brute-force enumeration on
simulated per-stream rings, the padding ladder, and the argument checks, which raise before any device work."""
import random

import pytest
import torch

from vad_amd import stream_group as sg
from vad_amd.cad import CausalAnomalyDetector


@pytest.mark.parametrize("window", [1, 4])
@pytest.mark.parametrize("stride", ["1", "2", "window+1"])
@pytest.mark.parametrize("max_push", [1, 3])
def test_group_schedule_against_brute_force(window, stride, max_push):
    """Three streams, 300 pushes of random sizes 0..max_push (zeros included), on one array of 3 * cap slots that
    records which (stream, frame) each slot holds.  Per push: no destination is shared; every destination and every
    slot a window reads lies in its own stream's range; every window -- exactly those whose last frame the push
    brings, per stream in order -- finds the frames it names in its slots; windows <= frames."""
    stride = {"1": 1, "2": 2, "window+1": window + 1}[stride]
    S, cap = 3, window + max_push - 1
    clip0 = [3, 50, 1000]
    rng = random.Random(100 * window + 10 * stride + max_push)
    slots = [None] * (S * cap)
    seen, emitted = [0] * S, [0] * S
    pushes = windows = 0
    while pushes < 300:
        ks = [rng.randint(0, max_push) for _ in range(S)]
        if pushes % 7 == 0:
            ks[rng.randrange(S)] = 0
        dst, rows = sg.group_schedule(seen, emitted, ks, window, stride, cap=cap, clip0=clip0)
        pushes += 1
        assert len(dst) == sum(ks) and len(set(dst)) == len(dst)
        assert len(rows) <= len(dst)
        # the frames go where the table says, in stream order
        it = iter(dst)
        for s in range(S):
            for g in range(seen[s], seen[s] + ks[s]):
                d = next(it)
                assert s * cap <= d < (s + 1) * cap
                slots[d] = (s, g)
        # brute force: per stream, the windows whose last frame is among the new ones
        want = [(s, w) for s in range(S) for w in range(seen[s] + ks[s])
                if seen[s] <= w * stride + window - 1 < seen[s] + ks[s]]
        assert len(rows) == len(want)
        for (base, first, key), (s, w) in zip(rows, want):
            assert base == s * cap and 0 <= first < cap
            assert key == clip0[s] + w
            for t in range(window):
                sl = first + t
                sl = sl - cap if sl >= cap else sl  # (wrapped once, as the kernels do)
                assert 0 <= sl < cap
                assert slots[base + sl] == (s, w * stride + t), f"stream {s} window {w} frame {t}"
        for s in range(S):
            seen[s] += ks[s]
            emitted[s] += sum(1 for q, _ in want if q == s)
        windows += len(want)
    assert windows > 0
    for s in range(S):
        assert emitted[s] == ((seen[s] - window) // stride + 1 if seen[s] >= window else 0)


def test_group_schedule_defaults_to_clip0_zero():
    dst, rows = sg.group_schedule([3, 0], [0, 0], [1, 1], 4, 1, cap=4)
    assert dst == [3, 4] and rows == [(0, 0, 0)]
    # the second window of stream 1 starts at slot 1 of its ring and wraps
    dst, rows = sg.group_schedule([4, 4], [1, 1], [0, 1], 4, 1, cap=4)
    assert dst == [4] and rows == [(4, 1, 1)]


def test_padding_ladder():
    """Plan sizes are the powers of two below num_streams * max_push and that product itself."""
    assert [sg.padded_frames(f, 12) for f in range(1, 13)] == [1, 2, 4, 4, 8, 8, 8, 8, 12, 12, 12, 12]
    assert [sg.padded_frames(f, 8) for f in range(1, 9)] == [1, 2, 4, 4, 8, 8, 8, 8]
    assert sg.padded_frames(1, 1) == 1
    for limit in (1, 5, 16, 96):
        ladder = {sg.padded_frames(f, limit) for f in range(1, limit + 1)}
        assert len(ladder) <= (limit - 1).bit_length() + 1
        assert all(f <= sg.padded_frames(f, limit) <= limit for f in range(1, limit + 1))


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return CausalAnomalyDetector().eval()


@pytest.mark.parametrize("kw, text", [
    (dict(num_streams=0), "num_streams"),
    (dict(num_streams=2, window=0), "window"),
    (dict(num_streams=2, stride=0), "stride"),
    (dict(num_streams=2, max_push=1.5), "max_push"),
    (dict(num_streams=2, clip0=[1, 2, 3]), "clip0"),
])
def test_open_stream_group_rejects_bad_arguments(model, kw, text):
    with pytest.raises(ValueError, match=text):
        model.open_stream_group(**kw)


def _f(k, c=1, h=32, w=32):
    return torch.zeros(k, c, h, w)


@pytest.mark.parametrize("frames, text", [
    ([_f(1)], "num_streams = 2"),
    ([_f(1), _f(1), _f(1)], "num_streams = 2"),
    (_f(2), "num_streams = 2"),
    ([_f(3), _f(1)], "max_push"),
    ([_f(1), _f(1, h=48)], "frame size"),
    ([_f(1), _f(1, c=3)], "single-channel"),
    ([_f(1), torch.zeros(1, 32, 32)], "shape"),
    ([None, None], "no stream brought a frame"),
    ([_f(0), None], "no stream brought a frame"),
])
def test_push_rejects_bad_frames_without_a_device(model, frames, text):
    g = model.open_stream_group(2, window=4, max_push=2)
    with pytest.raises(ValueError, match=text):
        g.push(frames)
    assert g.frames_seen == [0, 0] and g.windows_emitted == [0, 0] and g.frame_size is None


def test_push_rejects_a_frame_size_other_than_the_groups(model):
    # (the first push needs a device; its effect on the check is the recorded frame size)
    with pytest.raises(ValueError, match="frame size"):
        sg.check_group_push(model, [_f(1, h=48), None], 2, 2, (32, 32))
    chunks, ks, size = sg.check_group_push(model, [None, _f(2)], 2, 2, None)
    assert chunks[0] is None and chunks[1].shape == (2, 1, 32, 32) and ks == [0, 2] and size == (32, 32)


def test_group_rejects_training_mode_and_bf16(model):
    g = model.open_stream_group(2, window=4)
    x = [_f(1), _f(1)]
    model.train()
    try:
        with pytest.raises(ValueError, match="eval mode"):
            model.open_stream_group(2, window=4)
        with pytest.raises(ValueError, match="eval mode"):
            g.push(x)
    finally:
        model.eval()
    model.set_compute_dtype(torch.bfloat16)
    try:
        with pytest.raises(ValueError, match="fp32 only"):
            model.open_stream_group(2, window=4)
        with pytest.raises(ValueError, match="fp32 only"):
            g.push(x)
    finally:
        model.set_compute_dtype(torch.float32)


def test_group_counters_ring_sizes_and_reset(model):
    g = model.open_stream_group(3, window=16, max_push=8, clip0=(3, 50, 1000))
    assert (g.cap, g.total_slots, g.max_frames) == (23, 69, 24)
    assert g.clip0 == [3, 50, 1000] and model.open_stream_group(2, clip0=7).clip0 == [7, 7]
    g.frames_seen, g.windows_emitted = [30, 31, 32], [15, 16, 17]
    g.reset(1)
    assert g.frames_seen == [30, 0, 32] and g.windows_emitted == [15, 0, 17]
    g.reset()
    assert g.frames_seen == [0, 0, 0] and g.windows_emitted == [0, 0, 0]
