"""Scoring many live streams of one frame size with CausalAnomalyDetector in shared launches (eval mode, forward
only, fp32).

One CadStream per camera costs one launch-bound push per camera.  In eval mode every per-frame result depends on its
frame alone and every per-window result on its window alone, so a group runs the frames of all its streams through one
per-frame pass and all the windows they complete through one per-window pass (vad_cad_frames_forward_group /
vad_cad_windows_forward_group).

Memory is one FrameCache(num_streams * cap) allocation, cap = window + max_push - 1: ring s occupies slots
``s * cap .. (s + 1) * cap - 1`` and frame g of stream s lives in slot ``s * cap + g mod cap``; stream.py's argument
for why cap slots suffice holds per stream.  Where a frame goes and which slots a window reads are tables built on the
host (group_schedule), validated by the library and copied to the device once per stage.

The ``F = sum of k_s`` frames of a push are zero-padded to the next power of two (at most num_streams * max_push), the
padding frames being stored nowhere, so a group creates at most ``ceil(log2(num_streams * max_push)) + 1`` plans with
their workspaces instead of one per distinct F; the price is the per-frame stage of up to F - 1 frames of zeros.

Stream s returns what ``model.open_stream(window, stride, max_push=max_push, seed=seed, step=step,
clip0=clip0[s])`` returns for the same history of frames.
"""
from __future__ import annotations

import torch

from . import _native as nat
from .stream import _positive_int, check_frame_size, check_model, stream_schedule
from .video import MAX_DET, NUM_FACTORS, cache_field


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


def check_group_push(model, frames, num_streams, max_push, frame_size):
    """The ValueErrors of CadStreamGroup.push, raised before any device work.  Returns (chunks, ks, (H, W)): per stream
    the frames as (k_s, 1, H, W) or None where k_s = 0."""
    check_model(model)
    if not isinstance(frames, (list, tuple)) or len(frames) != num_streams:
        got = f"{len(frames)} entries" if isinstance(frames, (list, tuple)) else type(frames).__name__
        raise ValueError(f"push: a list or tuple of num_streams = {num_streams} entries (frames (k, 1, H, W) or None), "
                         f"got {got}")
    chunks, ks = [], []
    for s, x in enumerate(frames):
        if x is None:
            chunks.append(None)
            ks.append(0)
            continue
        if not isinstance(x, torch.Tensor) or x.dim() != 4:
            raise ValueError(f"push: stream {s}: frames of shape (k, 1, H, W) or None, got "
                             f"{tuple(getattr(x, 'shape', ()))}")
        if x.shape[1] != 1:
            raise ValueError(f"push: stream {s}: ResNetBackbone here takes single-channel frames "
                             "(input_channels=1, cad:515)")
        k = x.shape[0]
        if k > max_push:
            raise ValueError(f"push: stream {s}: at most max_push = {max_push} frames per push, got {k}")
        if k > 0:
            if frame_size is None:
                frame_size = tuple(x.shape[2:])
            elif tuple(x.shape[2:]) != tuple(frame_size):
                raise ValueError(f"push: stream {s}: frame size {tuple(x.shape[2:])} differs from the group's "
                                 f"{tuple(frame_size)}")
        chunks.append(x if k > 0 else None)
        ks.append(k)
    if sum(ks) == 0:
        raise ValueError("push: no stream brought a frame")
    return chunks, ks, frame_size


def check_group_push_u8(model, frames, num_streams, max_push, check_model=check_model, color=None):
    """The ValueErrors of a group's push_u8, raised before any device work.  Returns (chunks, ks): per stream the
    frames as uint8 (k_s, Hs_s, Ws_s) -- with a colour format (k_s, Hs_s, Ws_s, C) -- each stream at its own source
    size, or None where k_s = 0."""
    from .data import check_u8_frames
    check_model(model)
    if not isinstance(frames, (list, tuple)) or len(frames) != num_streams:
        got = f"{len(frames)} entries" if isinstance(frames, (list, tuple)) else type(frames).__name__
        raise ValueError(f"push_u8: a list or tuple of num_streams = {num_streams} entries (uint8 frames (k, Hs, Ws) "
                         f"or (k, 1, Hs, Ws), or None), got {got}")
    chunks, ks = [], []
    for s, x in enumerate(frames):
        if x is None:
            chunks.append(None)
            ks.append(0)
            continue
        x = check_u8_frames(x, f"push_u8: stream {s}", color)
        k = x.shape[0]
        if k > max_push:
            raise ValueError(f"push_u8: stream {s}: at most max_push = {max_push} frames per push, got {k}")
        chunks.append(x if k > 0 else None)
        ks.append(k)
    if sum(ks) == 0:
        raise ValueError("push_u8: no stream brought a frame")
    return chunks, ks


class CadStreamGroup:
    """CausalAnomalyDetector.open_stream_group's result: num_streams rings in one cache, two counters per stream, one
    device table and its pinned host image.  As with CadStream the model's plans are borrowed for the duration of a
    push only."""

    def __init__(self, model, num_streams, window=16, stride=1, *, max_push=1, seed=0, step=0, clip0=0,
                 frame_size=None):
        self.num_streams = _positive_int("num_streams", num_streams)
        self.window = _positive_int("window", window)
        self.stride = _positive_int("stride", stride)
        self.max_push = _positive_int("max_push", max_push)
        check_model(model)
        self.model = model
        self.cap = self.window + self.max_push - 1
        self.total_slots = self.num_streams * self.cap
        self.max_frames = self.num_streams * self.max_push
        self.seed, self.step = int(seed), int(step)
        if isinstance(clip0, (int, float)):
            clip0 = [clip0] * self.num_streams
        if len(clip0) != self.num_streams:
            raise ValueError(f"open_stream_group: clip0 must be an int or {self.num_streams} ints, got {len(clip0)}")
        self.clip0 = [int(c) for c in clip0]
        # (H, W) of the frames the model sees: given, or fixed by the first push (a u8 push: its first source's size)
        self.frame_size = check_frame_size(frame_size, "open_stream_group")
        self._ring = None
        self._ingest = self._u8 = None  # push_u8's U8Ingest and its fp32 buffer of max_frames frames
        self.frames_seen = [0] * self.num_streams
        self.windows_emitted = [0] * self.num_streams

    def reset(self, s=None):
        """Stream s, or every stream, back to frame 0 and window 0; the rings are kept (nothing of them is read before
        it is written again)."""
        for i in range(self.num_streams) if s is None else [s]:
            self.frames_seen[i] = 0
            self.windows_emitted[i] = 0

    def _allocate(self, L, dev):
        nfl = L.vad_cad_frame_cache_floats(self.total_slots)
        nb = L.vad_cad_group_table_bytes(self.max_frames, self.max_frames)
        if nfl < 0 or nb < 0:
            nat.check(1)
        self._ring = torch.zeros(nfl, dtype=torch.float32, device=dev)
        # the device table (destinations as int32 from byte 0) and the pinned host tables the library copies from; a
        # push ends with host reads on the stream, so the next one never overwrites a table the device has yet to copy
        self._table = torch.zeros((nb + 3) // 4, dtype=torch.int32, device=dev)
        self._h_dst = torch.empty(self.max_frames, dtype=torch.int32).pin_memory()
        self._h_win = torch.empty(self.max_frames, 3, dtype=torch.int64).pin_memory()

    def push(self, frames) -> list:
        """frames: a sequence of num_streams entries, entry s the next 0 <= k_s <= max_push frames of stream s as
        (k_s, 1, H, W) on the device, or None.  Returns one CadStream.push dict per stream: empty tensors where the
        stream completed no window, no detections where it pushed nothing."""
        chunks, ks, size = check_group_push(self.model, frames, self.num_streams, self.max_push, self.frame_size)
        live = [x for x in chunks if x is not None]
        for x in live:
            nat.require_hip(x)
        F = sum(ks)
        P = padded_frames(F, self.max_frames)
        # the frames of all streams and the padding, in one copy
        parts = [x.float() for x in live]
        if P > F:
            parts.append(torch.zeros(P - F, 1, *size, dtype=torch.float32, device=live[0].device))
        x = parts[0].contiguous() if len(parts) == 1 else torch.cat(parts)
        return self._push(x, ks, size)

    def push_u8(self, frames, color=None) -> list:
        """frames: a sequence of num_streams entries, entry s the next 0 <= k_s <= max_push frames of camera s as uint8
        (k_s, Hs, Ws) or (k_s, 1, Hs, Ws), or None; cameras may differ in source size and in where their frames lie
        (device, pinned host memory read in place, pageable host memory).  One table-form launch resizes every frame
        to the group's frame size as data.resize_u8 does, normalises it as (u8 - 0.5) / 0.5 and writes the zero
        padding, into a buffer the group owns (data.U8Ingest.table); the rest is push: push_u8 returns what push
        returns for the same frames converted on the host.  Without frame_size the first push fixes it to the size of
        its first source.  With color ("rgb", "bgr", "rgbx" or "bgrx") every camera brings packed colour pixels,
        uint8 (k_s, Hs, Ws, 3) or (k_s, Hs, Ws, 4) -- one format for the whole call -- and the same launch takes their
        grey first (data.luma_u8, PIL's convert("L"))."""
        from .data import U8Ingest, ingest_device
        chunks, ks = check_group_push_u8(self.model, frames, self.num_streams, self.max_push, color=color)
        live = [x for x in chunks if x is not None]
        dev = ingest_device(self.model, live, "push_u8")
        size = self.frame_size or tuple(live[0].shape[1:3])
        if self._ingest is None:
            self._ingest = U8Ingest(dev)
            self._u8 = torch.empty(self.max_frames, 1, *size, dtype=torch.float32, device=dev)
        P = padded_frames(sum(ks), self.max_frames)
        x = self._ingest.table(live, P, size, 0, out=self._u8[:P], capacity=self.max_frames, color=color)
        return self._push(x, ks, size)

    def _push(self, x, ks, size) -> list:
        """push's body: x (P, 1, H, W), the sum(ks) frames in stream order, then zeros."""
        model, T, stride, cap, S = self.model, self.window, self.stride, self.cap, self.num_streams
        eng = model.engine()
        L = nat.lib()
        dev = eng.device
        stream = nat.stream_of(dev)
        if self._ring is None:
            self._allocate(L, dev)
            self.frame_size = size
        ring, H, W = self._ring, size[0], size[1]
        F, P = sum(ks), x.shape[0]
        dst, rows = group_schedule(self.frames_seen, self.windows_emitted, ks, T, stride, cap=cap, clip0=self.clip0)
        nw = len(rows)
        self._h_dst[:P] = torch.tensor(dst + [-1] * (P - F), dtype=torch.int32)
        # a forward armed for another input must not outlive this call (CadEngine.input_ready)
        armed, eng._armed = getattr(eng, "_armed", None), None
        if armed is not None:
            nat.check(L.vad_cad_set_option(armed.h, b"input_armed", 0))
        # (the plan's activations are overwritten: a backward still pending on an earlier forward must not read them)
        eng.generation += 1
        pl = eng.plan(P, 1, H, W)
        eng._set_stem_grad(pl)
        eng._check_images(pl)
        nat.check(L.vad_cad_frames_forward_group(pl.h, x.data_ptr(), self.total_slots, ring.data_ptr(),
                                                 self._h_dst.data_ptr(), self._table.data_ptr(), stream))
        o = dict(final=torch.empty(nw, device=dev), probs=torch.empty(nw, 2, device=dev),
                 causal=torch.empty(nw, device=dev), kl=torch.empty(nw, device=dev),
                 z=torch.empty(nw, MAX_DET, NUM_FACTORS, device=dev),
                 adj=torch.empty(nw, NUM_FACTORS, NUM_FACTORS, device=dev),
                 nmax=torch.empty(nw, dtype=torch.int32, device=dev))
        if nw > 0:
            self._h_win[:nw] = torch.tensor(rows, dtype=torch.int64)
            nat.check(L.vad_cad_windows_forward_group(
                pl.h, ring.data_ptr(), self.total_slots, cap, T, self._h_win.data_ptr(), nw, self._table.data_ptr(),
                self.seed & ((1 << 64) - 1), self.step, o["final"].data_ptr(), o["probs"].data_ptr(),
                o["causal"].data_ptr(), o["kl"].data_ptr(), o["z"].data_ptr(), o["adj"].data_ptr(),
                o["nmax"].data_ptr(), stream))
        # the pushed frames' boxes and counts, gathered through the destinations the device table already holds
        idx = self._table[:F]
        boxes = cache_field(ring, self.total_slots, "boxes").index_select(0, idx)
        cnt = cache_field(ring, self.total_slots, "counts").index_select(0, idx).tolist()
        nm = o["nmax"].tolist()
        outs, f0, r0 = [], 0, 0
        for s in range(S):
            _, widx0, n = stream_schedule(self.frames_seen[s], self.windows_emitted[s], ks[s], T, stride)
            r1 = r0 + n
            outs.append({
                "anomaly_scores": o["final"][r0:r1],
                "direct_predictions": o["probs"][r0:r1],
                "causal_anomaly_scores": o["causal"][r0:r1],
                "kl_losses": o["kl"][r0:r1],
                "adjacency_matrices": o["adj"][r0:r1],
                "causal_factors": [o["z"][w, :nm[w]] for w in range(r0, r1)],
                "detections": [boxes[f, :cnt[f]] for f in range(f0, f0 + ks[s])],
                "window_starts": (widx0 + torch.arange(n, dtype=torch.int64)) * stride,
            })
            self.frames_seen[s] += ks[s]
            self.windows_emitted[s] = widx0 + n
            f0 += ks[s]
            r0 = r1
        return outs
