"""Scoring many live streams of one frame size with CausalAnomalyDetector in shared launches (eval mode, forward
only, fp32).

One CadStream per camera costs one launch-bound push per camera.  In eval mode every per-frame result depends on its
frame alone and every per-window result on its window alone, so a group runs the frames of all its streams through one
per-frame pass and all the windows they complete through one per-window pass (vad_cad_frames_forward_group /
vad_cad_windows_forward_group).

Memory is one FrameCache(num_streams * cap) allocation, cap = window + max_push - 1: ring s occupies slots
``s * cap .. (s + 1) * cap - 1`` and frame g of stream s lives in slot ``s * cap + g mod cap``; stream.py's argument
for why cap slots suffice holds per stream.  Where a frame goes and which slots a window reads are tables built on the
host (stream_util.group_schedule, held in a stream_util.GroupTables), validated by the library (csrc/group_table.h) and
copied to the device once per stage.

The ``F = sum of k_s`` frames of a push are zero-padded to the next power of two (at most num_streams * max_push), the
padding frames being stored nowhere, so a group creates at most ``ceil(log2(num_streams * max_push)) + 1`` plans with
their workspaces instead of one per distinct F; the price is the per-frame stage of up to F - 1 frames of zeros.

Stream s returns what ``model.open_stream(window, stride, max_push=max_push, seed=seed, step=step,
clip0=clip0[s])`` returns for the same history of frames.
"""
from __future__ import annotations

import torch

from . import _native as nat
from .stream import check_model
from .stream_util import (GroupTables, _positive_int, check_frame_size, gather_padded, group_schedule,  # noqa: F401
                          padded_frames, per_stream, stream_schedule, u8_buffer, walk_group_frames,
                          walk_group_frames_u8)
from .video import MAX_DET, NUM_FACTORS, cache_field


def check_group_push(model, frames, num_streams, max_push, frame_size):
    """The ValueErrors of CadStreamGroup.push, raised before any device work.  Returns (chunks, ks, (H, W)): per stream
    the frames as (k_s, 1, H, W) or None where k_s = 0."""
    check_model(model)
    size = [frame_size]  # the group's, or that of the first frames seen

    def check_one(s, x):
        if not isinstance(x, torch.Tensor) or x.dim() != 4:
            raise ValueError(f"push: stream {s}: frames of shape (k, 1, H, W) or None, got "
                             f"{tuple(getattr(x, 'shape', ()))}")
        if x.shape[1] != 1:
            raise ValueError(f"push: stream {s}: ResNetBackbone here takes single-channel frames "
                             "(input_channels=1, cad:515)")
        if 0 < x.shape[0] <= max_push:  # (more than max_push frames: the walk's error comes first)
            if size[0] is None:
                size[0] = tuple(x.shape[2:])
            elif tuple(x.shape[2:]) != tuple(size[0]):
                raise ValueError(f"push: stream {s}: frame size {tuple(x.shape[2:])} differs from the group's "
                                 f"{tuple(size[0])}")
        return x

    chunks, ks = walk_group_frames(frames, num_streams, max_push, "push", check_one, "frames (k, 1, H, W) or None")
    return chunks, ks, size[0]


def check_group_push_u8(model, frames, num_streams, max_push, check_model=check_model, color=None):
    """The ValueErrors of a group's push_u8, raised before any device work: stream_util.walk_group_frames_u8's."""
    check_model(model)
    return walk_group_frames_u8(frames, num_streams, max_push, color)


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
        if nfl < 0:
            nat.check(1)
        self._ring = torch.zeros(nfl, dtype=torch.float32, device=dev)
        # the device table and the pinned host tables the library copies from (stream_util.GroupTables); a push ends
        # with host reads on the stream, so the next one never overwrites a table the device has yet to copy
        self._tables = GroupTables(L.vad_cad_group_table_bytes, self.max_frames, 3, dev)

    def push(self, frames) -> list:
        """frames: a sequence of num_streams entries, entry s the next 0 <= k_s <= max_push frames of stream s as
        (k_s, 1, H, W) on the device, or None.  Returns one CadStream.push dict per stream: empty tensors where the
        stream completed no window, no detections where it pushed nothing."""
        chunks, ks, size = check_group_push(self.model, frames, self.num_streams, self.max_push, self.frame_size)
        live = [x for x in chunks if x is not None]
        for x in live:
            nat.require_hip(x)
        F = sum(ks)
        return self._push(gather_padded(live, F, padded_frames(F, self.max_frames), (1, *size)), ks, size)

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
        from .data import ingest_device
        chunks, ks = check_group_push_u8(self.model, frames, self.num_streams, self.max_push, color=color)
        live = [x for x in chunks if x is not None]
        dev = ingest_device(self.model, live, "push_u8")
        size = self.frame_size or tuple(live[0].shape[1:3])
        ingest, buf = u8_buffer(self, dev, self.max_frames, size)
        P = padded_frames(sum(ks), self.max_frames)
        x = ingest.table(live, P, size, 0, out=buf[:P], capacity=self.max_frames, color=color)
        return self._push(x, ks, size)

    def _push(self, x, ks, size) -> list:
        """push's body: x (P, 1, H, W), the sum(ks) frames in stream order, then zeros."""
        model, T, stride, cap = self.model, self.window, self.stride, self.cap
        eng = model.engine()
        L = nat.lib()
        dev = eng.device
        stream = nat.stream_of(dev)
        if self._ring is None:
            self._allocate(L, dev)
            self.frame_size = size
        ring, tables, H, W = self._ring, self._tables, size[0], size[1]
        F, P = sum(ks), x.shape[0]
        dst, rows = group_schedule(self.frames_seen, self.windows_emitted, ks, T, stride, cap=cap, clip0=self.clip0)
        nw = len(rows)
        tables.fill_dst(dst, P)
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
                                                 tables.h_dst.data_ptr(), tables.dev.data_ptr(), stream))
        o = dict(final=torch.empty(nw, device=dev), probs=torch.empty(nw, 2, device=dev),
                 causal=torch.empty(nw, device=dev), kl=torch.empty(nw, device=dev),
                 z=torch.empty(nw, MAX_DET, NUM_FACTORS, device=dev),
                 adj=torch.empty(nw, NUM_FACTORS, NUM_FACTORS, device=dev),
                 nmax=torch.empty(nw, dtype=torch.int32, device=dev))
        if nw > 0:
            tables.fill_windows(rows)
            nat.check(L.vad_cad_windows_forward_group(
                pl.h, ring.data_ptr(), self.total_slots, cap, T, tables.h_win.data_ptr(), nw, tables.dev.data_ptr(),
                self.seed & ((1 << 64) - 1), self.step, o["final"].data_ptr(), o["probs"].data_ptr(),
                o["causal"].data_ptr(), o["kl"].data_ptr(), o["z"].data_ptr(), o["adj"].data_ptr(),
                o["nmax"].data_ptr(), stream))
        # the pushed frames' boxes and counts, gathered through the destinations the device table already holds
        idx = tables.dev[:F]
        boxes = cache_field(ring, self.total_slots, "boxes").index_select(0, idx)
        cnt = cache_field(ring, self.total_slots, "counts").index_select(0, idx).tolist()
        nm = o["nmax"].tolist()
        return [{
            "anomaly_scores": o["final"][r0:r1],
            "direct_predictions": o["probs"][r0:r1],
            "causal_anomaly_scores": o["causal"][r0:r1],
            "kl_losses": o["kl"][r0:r1],
            "adjacency_matrices": o["adj"][r0:r1],
            "causal_factors": [o["z"][w, :nm[w]] for w in range(r0, r1)],
            "detections": [boxes[f, :cnt[f]] for f in range(f0, f1)],
            "window_starts": (widx0 + torch.arange(n, dtype=torch.int64)) * stride,
        } for s, f0, f1, r0, r1, widx0, n in per_stream(self.frames_seen, self.windows_emitted, ks, T, stride)]
