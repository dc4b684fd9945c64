"""What the four stream classes (stream.py, stream_group.py, ae_stream.py, ae_stream_group.py) share: argument checks,
the push schedules, and a group's tables and bookkeeping.  Nothing here knows a model: each class keeps its own _push,
a sequence of native calls read top to bottom, and calls these for the parts that do not depend on what is scored.
"""
from __future__ import annotations

import torch

from . import _native as nat


def _positive_int(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or int(v) != v or v < 1:
        raise ValueError(f"open_stream: {name} must be an integer >= 1, got {v!r}")
    return int(v)


def check_frame_size(frame_size, what="open_stream"):
    if frame_size is None:
        return None
    try:
        size = tuple(int(v) for v in frame_size)
        ok = len(size) == 2 and size == tuple(frame_size) and min(size) >= 1
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{what}: frame_size must be None or (H, W), two integers >= 1, got {frame_size!r}")
    return size


def stream_schedule(frames_seen: int, windows_emitted: int, k: int, window: int, stride: int):
    """The windows a push of k frames completes, for a stream that has taken frames_seen frames and emitted
    windows_emitted windows: (first_frame, widx0, nw) -- nw windows, window i of the batch being window widx0 + i of
    the stream, frames first_frame + i * stride + t.  Window w is complete once frame w * stride + window - 1 is in."""
    total = frames_seen + k
    complete = (total - window) // stride + 1 if total >= window else 0
    return windows_emitted * stride, windows_emitted, complete - windows_emitted


def group_schedule(frames_seen, windows_emitted, ks, window, stride, *, cap, clip0=None):
    """The tables of one push in which stream s, having taken frames_seen[s] frames and emitted windows_emitted[s]
    windows, brings ks[s] >= 0 frames to its ring of cap slots: (dst, rows), both in stream order.  dst: the absolute
    slot of every pushed frame, ``s * cap + g mod cap``.  rows: (base, first, key) of every window the push completes,
    per stream in window order -- base = s * cap, first = the slot of the window's first frame within the ring,
    key = clip0[s] + the window's index in its stream.  A push completes at most sum(ceil(k_s / stride)) <= sum(k_s)
    windows."""
    dst, rows = [], []
    for s, k in enumerate(ks):
        base = s * cap
        dst += [base + g % cap for g in range(frames_seen[s], frames_seen[s] + k)]
        first, widx0, nw = stream_schedule(frames_seen[s], windows_emitted[s], k, window, stride)
        c0 = 0 if clip0 is None else clip0[s]
        rows += [(base, (first + i * stride) % cap, c0 + widx0 + i) for i in range(nw)]
    return dst, rows


def padded_frames(f: int, limit: int) -> int:
    """The plan size of a push of 1 <= f <= limit frames: the next power of two, capped at limit."""
    return min(1 << (f - 1).bit_length(), limit)


def check_push_u8(model, frames, max_push, what="push_u8", color=None) -> torch.Tensor:
    """The ValueErrors of a stream's push_u8, raised before any device work; returns the frames as (k, Hs, Ws), with a
    colour format as (k, Hs, Ws, C)."""
    from .data import check_u8_frames
    x = check_u8_frames(frames, what, color)
    k = x.shape[0]
    if k < 1 or k > max_push:
        raise ValueError(f"{what}: between 1 and max_push = {max_push} frames per push, got {k}")
    return x


def walk_group_frames(frames, num_streams, max_push, what, check_one, entry):
    """The ValueErrors every group push raises over its list of per-stream frames, before any device work.
    check_one(s, x) checks stream s's entry x (not None) for its model and returns it in the form the push works on;
    entry says what an entry may be in the error text.  Returns (chunks, ks): per stream the checked frames, or None
    where k_s = 0."""
    if not isinstance(frames, (list, tuple)) or len(frames) != num_streams:
        got = f"{len(frames)} entries" if isinstance(frames, (list, tuple)) else type(frames).__name__
        raise ValueError(f"{what}: a list or tuple of num_streams = {num_streams} entries ({entry}), got {got}")
    chunks, ks = [], []
    for s, x in enumerate(frames):
        if x is None:
            chunks.append(None)
            ks.append(0)
            continue
        x = check_one(s, x)
        k = x.shape[0]
        if k > max_push:
            raise ValueError(f"{what}: stream {s}: at most max_push = {max_push} frames per push, got {k}")
        chunks.append(x if k > 0 else None)
        ks.append(k)
    if sum(ks) == 0:
        raise ValueError(f"{what}: no stream brought a frame")
    return chunks, ks


def walk_group_frames_u8(frames, num_streams, max_push, color=None):
    """walk_group_frames for a group's push_u8: per stream the frames as uint8 (k_s, Hs_s, Ws_s) -- with a colour
    format (k_s, Hs_s, Ws_s, C) -- each stream at its own source size."""
    from .data import check_u8_frames
    return walk_group_frames(frames, num_streams, max_push, "push_u8",
                             lambda s, x: check_u8_frames(x, f"push_u8: stream {s}", color),
                             "uint8 frames (k, Hs, Ws) or (k, 1, Hs, Ws), or None")


def gather_padded(live, F, P, frame_shape):
    """The F frames of the chunks in live as fp32, then P - F frames of zeros of frame_shape = (1, H, W): (P, 1, H, W),
    contiguous, in one copy."""
    parts = [x.float() for x in live]
    if P > F:
        parts.append(torch.zeros(P - F, *frame_shape, dtype=torch.float32, device=live[0].device))
    return parts[0].contiguous() if len(parts) == 1 else torch.cat(parts)


def per_stream(frames_seen, windows_emitted, ks, window, stride):
    """How the results of one group push split among its streams: yields (s, f0, f1, r0, r1, widx0, n) per stream --
    frames f0 .. f1 - 1 of the push and rows r0 .. r1 - 1 of its window outputs are stream s's, the n = r1 - r0 windows
    being windows widx0 .. of that stream -- and advances frames_seen[s] and windows_emitted[s] past the push."""
    f0 = r0 = 0
    for s, k in enumerate(ks):
        _, widx0, n = stream_schedule(frames_seen[s], windows_emitted[s], k, window, stride)
        frames_seen[s] += k
        windows_emitted[s] = widx0 + n
        yield s, f0, f0 + k, r0, r0 + n, widx0, n
        f0 += k
        r0 += n


def u8_buffer(obj, dev, n, size):
    """push_u8's state on a stream or group obj, created at its first use: obj._ingest, a data.U8Ingest on dev, and
    obj._u8, the fp32 buffer of n frames of size (H, W) it writes to.  Returns both."""
    if obj._ingest is None:
        from .data import U8Ingest
        obj._ingest = U8Ingest(dev)
        obj._u8 = torch.empty(n, 1, *size, dtype=torch.float32, device=dev)
    return obj._ingest, obj._u8


class GroupTables:
    """The tables of a stream group: dev, the device table of table_bytes = the model's vad_*_group_table_bytes
    (csrc/group_table.h), and the pinned host images the library copies from, h_dst (max_frames int32) and h_win
    (max_frames rows of win_cols int64).  When one may be written again is its owner's business (AeStreamGroup)."""

    def __init__(self, table_bytes, max_frames, win_cols, dev):
        nb = table_bytes(max_frames, max_frames)
        if nb < 0:
            nat.check(1)
        self.dev = torch.zeros((nb + 3) // 4, dtype=torch.int32, device=dev)
        self.h_dst = torch.empty(max_frames, dtype=torch.int32).pin_memory()
        self.h_win = torch.empty(max_frames, win_cols, dtype=torch.int64).pin_memory()

    def fill_dst(self, dst, P):
        """The destinations of a push's frames, then -1 (stored nowhere) up to the plan's P frames."""
        self.h_dst[:P] = torch.tensor(dst + [-1] * (P - len(dst)), dtype=torch.int32)

    def fill_windows(self, rows):
        self.h_win[:len(rows)] = torch.tensor(rows, dtype=torch.int64)
