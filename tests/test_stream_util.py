"""stream_util without a device: the per-stream split of a group push against a transcription of the loop both group
classes ended their _push with, the list walk's messages, and the padding of a push."""
import pytest
import torch

from vad_amd import stream_util as su


def _split_loop(frames_seen, windows_emitted, ks, window, stride):
    """The loop CadStreamGroup._push and AeStreamGroup._push both ended with, transcribed: the slices it took and the
    counters it left."""
    out, f0, r0 = [], 0, 0
    for s in range(len(ks)):
        _, widx0, n = su.stream_schedule(frames_seen[s], windows_emitted[s], ks[s], window, stride)
        r1 = r0 + n
        out.append((s, f0, f0 + ks[s], r0, r1, widx0, n))
        frames_seen[s] += ks[s]
        windows_emitted[s] = widx0 + n
        f0 += ks[s]
        r0 = r1
    return out


@pytest.mark.parametrize("num_streams", [1, 3])
@pytest.mark.parametrize("window", [2, 3])
@pytest.mark.parametrize("stride", [1, 2])
def test_per_stream_is_the_loop_it_replaces(num_streams, window, stride):
    """Twelve consecutive pushes on the same counters, ks cycling through 0, 1 and max_push per stream out of phase:
    every stream takes 16 frames, several times its ring of cap = window + max_push - 1 <= 5 slots."""
    max_push = 3
    sizes = [0, 1, max_push, 1, max_push, 0]
    seen_a, emitted_a = [0] * num_streams, [0] * num_streams
    seen_b, emitted_b = [0] * num_streams, [0] * num_streams
    windows = 0
    for push in range(12):
        ks = [sizes[(push + 2 * s) % len(sizes)] for s in range(num_streams)]
        want = _split_loop(seen_b, emitted_b, ks, window, stride)
        got = list(su.per_stream(seen_a, emitted_a, ks, window, stride))
        assert got == want
        assert seen_a == seen_b and emitted_a == emitted_b
        assert got[-1][2] == sum(ks)
        windows += got[-1][4]
    assert windows > 0 and min(seen_a) == 16 > window + max_push - 1
    for s in range(num_streams):
        assert emitted_a[s] == (seen_a[s] - window) // stride + 1


def _f(k):
    return torch.zeros(k, 1, 4, 4)


def _walk(frames, num_streams=2, max_push=2, what="push", entry="frames (k, 1, H, W) or None"):
    return su.walk_group_frames(frames, num_streams, max_push, what, lambda s, x: x, entry)


@pytest.mark.parametrize("frames, got", [([_f(1)], "1 entries"), ([_f(1)] * 3, "3 entries"), ((), "0 entries"),
                                         (_f(2), "Tensor"), (None, "NoneType")])
@pytest.mark.parametrize("what, entry", [
    ("push", "frames (k, 1, H, W) or None"),
    ("push", "frames (k, 1, 64, 64) or None"),
    ("push_u8", "uint8 frames (k, Hs, Ws) or (k, 1, Hs, Ws), or None"),
])
def test_walk_rejects_a_wrong_length_or_a_non_list(frames, got, what, entry):
    with pytest.raises(ValueError) as e:
        _walk(frames, what=what, entry=entry)
    assert str(e.value) == f"{what}: a list or tuple of num_streams = 2 entries ({entry}), got {got}"


def test_walk_rejects_an_entry_over_max_push_and_all_empty_entries():
    with pytest.raises(ValueError) as e:
        _walk([_f(2), _f(3)])
    assert str(e.value) == "push: stream 1: at most max_push = 2 frames per push, got 3"
    with pytest.raises(ValueError) as e:
        _walk([_f(1), _f(5)], what="push_u8")
    assert str(e.value) == "push_u8: stream 1: at most max_push = 2 frames per push, got 5"
    for frames in ([None, None], [_f(0), None], (_f(0), _f(0))):
        with pytest.raises(ValueError) as e:
            _walk(frames)
        assert str(e.value) == "push: no stream brought a frame"
    with pytest.raises(ValueError) as e:
        _walk([None, None], what="push_u8")
    assert str(e.value) == "push_u8: no stream brought a frame"


def test_walk_returns_the_checked_frames_and_their_counts():
    seen = []

    def check_one(s, x):
        seen.append(s)
        return x + 1

    a, b = _f(2), _f(1)
    chunks, ks = su.walk_group_frames([a, None, _f(0), b], 4, 2, "push", check_one, "")
    assert ks == [2, 0, 0, 1] and seen == [0, 2, 3]
    assert chunks[1] is None and chunks[2] is None
    assert torch.equal(chunks[0], a + 1) and torch.equal(chunks[3], b + 1)
    with pytest.raises(KeyError):  # check_one's own errors pass through, before the max_push check
        su.walk_group_frames([_f(3)], 1, 2, "push", lambda s, x: {}[s], "")


def test_walk_u8_names_the_stream_and_the_u8_forms():
    u8 = torch.zeros(2, 5, 7, dtype=torch.uint8)
    chunks, ks = su.walk_group_frames_u8([None, u8[:, None]], 2, 2)
    assert ks == [0, 2] and chunks[0] is None and chunks[1].shape == (2, 5, 7)
    with pytest.raises(ValueError, match="^push_u8: stream 1"):
        su.walk_group_frames_u8([u8, u8.float()], 2, 2)
    with pytest.raises(ValueError) as e:
        su.walk_group_frames_u8([u8], 2, 2)
    assert str(e.value) == ("push_u8: a list or tuple of num_streams = 2 entries (uint8 frames (k, Hs, Ws) or "
                            "(k, 1, Hs, Ws), or None), got 1 entries")


def test_padded_frames_p_equal_to_f_and_greater():
    assert [su.padded_frames(f, 6) for f in range(1, 7)] == [1, 2, 4, 4, 6, 6]
    assert su.padded_frames(4, 4) == 4 and su.padded_frames(3, 4) == 4 and su.padded_frames(3, 3) == 3


def test_gather_padded_p_equal_to_f_and_greater():
    a = torch.arange(2 * 6, dtype=torch.float64).view(2, 1, 2, 3)
    b = -torch.arange(1 * 6, dtype=torch.float32).view(1, 1, 2, 3)
    frames = torch.cat([a.float(), b])
    x = su.gather_padded([a, b], 3, 3, (1, 2, 3))  # P = F, two chunks
    assert x.dtype == torch.float32 and x.is_contiguous() and torch.equal(x, frames)
    x = su.gather_padded([a, b], 3, 4, (1, 2, 3))  # P > F: zeros behind the frames
    assert x.shape == (4, 1, 2, 3) and torch.equal(x[:3], frames) and not x[3].any()
    x = su.gather_padded([b], 1, 4, (1, 2, 3))
    assert x.shape == (4, 1, 2, 3) and torch.equal(x[:1], b) and not x[1:].any()
    t = torch.arange(12, dtype=torch.float32).view(1, 1, 3, 4).transpose(2, 3)  # P = F, one chunk, not contiguous
    x = su.gather_padded([t], 1, 1, (1, 4, 3))
    assert x.is_contiguous() and torch.equal(x, t)

