"""Scoring many live streams with the memory autoencoder in shared launches (VideoAutoEncoder, eval mode, forward
only, fp32).

One AeStream per camera costs one launch-bound push per camera.  In eval mode every per-frame result depends on its
frame alone and every per-window result on its window alone, so a group runs the frames of all its streams through one
per-frame pass and all the windows they complete through one per-window pass (vad_ae_frames_forward_group /
vad_ae_windows_forward_group).

Memory is one ring allocation of ``num_streams * cap`` slots, cap = window + max_push - 1 (ae_stream.py's three arrays
lat, gx and pix over that many slots): ring s occupies slots ``s * cap .. (s + 1) * cap - 1`` of each array and frame
g of stream s lives in slot ``s * cap + g mod cap``; stream.py's argument for why cap slots suffice holds per stream.
Where a frame goes and which slots a window reads are tables built on the host (stream_group.group_schedule, whose
key column is not used here), validated by the library and copied to the device once per stage.

The ``F = sum of k_s`` frames of a push are zero-padded to the next power of two (at most num_streams * max_push), the
padding frames being stored nowhere, so a group creates at most ``ceil(log2(num_streams * max_push)) + 1`` plans
instead of one per distinct F (stream_group.padded_frames).

Stream s returns what ``model.open_stream(window, stride, max_push=max_push, return_reconstructions=...)`` returns
for the same history of frames.
"""
from __future__ import annotations

import torch

from . import _native as nat
from .ae_stream import check_model, ring_field
from .ae_video import HW, LATENT
from .stream import _positive_int, stream_schedule
from .stream_group import check_group_push_u8, group_schedule, padded_frames


def check_group_push(model, frames, num_streams, max_push):
    """The ValueErrors of AeStreamGroup.push, raised before any device work.  Returns (chunks, ks): per stream the
    frames as (k_s, 1, 64, 64), or None where k_s = 0."""
    check_model(model)
    if not isinstance(frames, (list, tuple)) or len(frames) != num_streams:
        got = f"{len(frames)} entries" if isinstance(frames, (list, tuple)) else type(frames).__name__
        raise ValueError(f"push: a list or tuple of num_streams = {num_streams} entries (frames (k, 1, 64, 64) or "
                         f"None), got {got}")
    chunks, ks = [], []
    for s, x in enumerate(frames):
        if x is None:
            chunks.append(None)
            ks.append(0)
            continue
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or tuple(x.shape[1:]) != (1, HW, HW):
            raise ValueError(f"push: stream {s}: frames of shape (k, 1, 64, 64) or None (the encoder's "
                             "Linear(128*4*4) fixes 64x64 single-channel frames, cad1:151), got "
                             f"{tuple(getattr(x, 'shape', ()))}")
        k = x.shape[0]
        if k > max_push:
            raise ValueError(f"push: stream {s}: at most max_push = {max_push} frames per push, got {k}")
        chunks.append(x if k > 0 else None)
        ks.append(k)
    if sum(ks) == 0:
        raise ValueError("push: no stream brought a frame")
    return chunks, ks


class AeStreamGroup:
    """VideoAutoEncoder.open_stream_group's result: num_streams rings in one allocation, two counters per stream, one
    device table and its pinned host images.  As with AeStream the model's (P, 1) plans are borrowed for the duration
    of a push only, and a push changes no parameter, BatchNorm buffer or counter and leaves the memory ring and
    memory_ptr alone."""

    def __init__(self, model, num_streams, window=16, stride=1, *, max_push=1, return_reconstructions=False):
        self.num_streams = _positive_int("num_streams", num_streams)
        self.window = _positive_int("window", window)
        self.stride = _positive_int("stride", stride)
        self.max_push = _positive_int("max_push", max_push)
        self.max_frames = self.num_streams * self.max_push
        # a push runs on a plan of up to max_frames frames, and a plan holds at most as many clips as the memory ring
        # has rows (vad_ae_create: update_memory writes B rows of it)
        if self.max_frames > model.memory_size:
            raise ValueError(f"open_stream_group: num_streams * max_push must be at most {model.memory_size} (the "
                             f"clips one plan may hold), got {self.num_streams} * {self.max_push} = {self.max_frames}")
        check_model(model)
        self.model = model
        self.return_reconstructions = bool(return_reconstructions)
        self.cap = self.window + self.max_push - 1
        self.total_slots = self.num_streams * self.cap
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
        nfl = L.vad_ae_ring_floats(self.total_slots)
        nb = L.vad_ae_group_table_bytes(self.max_frames, self.max_frames)
        if nfl < 0 or nb < 0:
            nat.check(1)
        self._ring = torch.zeros(nfl, dtype=torch.float32, device=dev)
        # the device table (destinations as int32 from byte 0) and the pinned host tables the library copies from.
        # Unlike CadStreamGroup.push, a push here ends with no host read, so it may return -- and the next push begin
        # -- before the device has copied the tables: _copied is recorded on the stream behind the last table copy of
        # a push, and the next push waits for it before it writes the host tables again (it has normally passed)
        self._table = torch.zeros((nb + 3) // 4, dtype=torch.int32, device=dev)
        self._h_dst = torch.empty(self.max_frames, dtype=torch.int32).pin_memory()
        self._h_win = torch.empty(self.max_frames, 2, dtype=torch.int64).pin_memory()
        self._copied = torch.cuda.Event()

    def push(self, frames) -> list:
        """frames: a sequence of num_streams entries, entry s the next 0 <= k_s <= max_push frames of stream s as
        (k_s, 1, 64, 64) on the device, or None.  Returns one AeStream.push dict per stream: empty tensors where the
        stream completed no window, frame_features (0, 64) where it pushed nothing."""
        chunks, ks = check_group_push(self.model, frames, self.num_streams, self.max_push)
        live = [x for x in chunks if x is not None]
        for x in live:
            nat.require_hip(x)
        F = sum(ks)
        P = padded_frames(F, self.max_frames)
        # the frames of all streams and the padding, in one copy
        parts = [x.to(torch.float32) for x in live]
        if P > F:
            parts.append(torch.zeros(P - F, 1, HW, HW, dtype=torch.float32, device=live[0].device))
        x = parts[0].contiguous() if len(parts) == 1 else torch.cat(parts)
        return self._push(x, ks)

    def push_u8(self, frames, color=None) -> list:
        """frames: a sequence of num_streams entries, entry s the next 0 <= k_s <= max_push frames of camera s as uint8
        (k_s, Hs, Ws) or (k_s, 1, Hs, Ws), or None; cameras may differ in source size and in where their frames lie
        (device, pinned host memory read in place, pageable host memory).  One table-form launch resizes every frame
        to 64x64 as data.resize_u8 does, normalises it as u8 / 255 clamped to 0.001..0.999 (cad1:110-114) and writes
        the zero padding, into a buffer the group owns (data.U8Ingest.table); the rest is push: push_u8 returns what
        push returns for the same frames converted on the host.  With color ("rgb", "bgr", "rgbx" or "bgrx") every camera brings packed colour pixels,
        uint8 (k_s, Hs, Ws, 3) or (k_s, Hs, Ws, 4) -- one format for the whole call -- and the same launch takes their
        grey first (data.luma_u8, PIL's convert("L"))."""
        from .data import U8Ingest, ingest_device
        chunks, ks = check_group_push_u8(self.model, frames, self.num_streams, self.max_push, check_model, color)
        live = [x for x in chunks if x is not None]
        dev = ingest_device(self.model, live, "push_u8")
        if self._ingest is None:
            self._ingest = U8Ingest(dev)
            self._u8 = torch.empty(self.max_frames, 1, HW, HW, dtype=torch.float32, device=dev)
        P = padded_frames(sum(ks), self.max_frames)
        x = self._ingest.table(live, P, (HW, HW), 2, out=self._u8[:P], capacity=self.max_frames, color=color)
        return self._push(x, ks)

    def _push(self, x, ks) -> list:
        """push's body: x (P, 1, 64, 64), the sum(ks) frames in stream order, then zeros."""
        T, stride, cap, S = self.window, self.stride, self.cap, self.num_streams
        eng = self.model.engine()
        L = nat.lib()
        dev = eng.device
        stream = eng.stream()
        if self._ring is None:
            self._allocate(L, dev)
        ring = self._ring
        F, P = sum(ks), x.shape[0]
        dst, rows = group_schedule(self.frames_seen, self.windows_emitted, ks, T, stride, cap=cap)
        nw = len(rows)
        self._copied.synchronize()  # (see _allocate: the device has the tables of the push before)
        self._h_dst[:P] = torch.tensor(dst + [-1] * (P - F), dtype=torch.int32)
        pl = eng.plan(P, 1)
        nat.check(L.vad_ae_frames_forward_group(pl.h, x.data_ptr(), self.total_slots, ring.data_ptr(),
                                                self._h_dst.data_ptr(), self._table.data_ptr(), stream))
        o = dict(seq=torch.empty(nw, LATENT, device=dev), err=torch.empty(nw, device=dev),
                 mem=torch.empty(nw, device=dev), score=torch.empty(nw, device=dev))
        recon = torch.empty(nw, 1, HW, HW, device=dev) if self.return_reconstructions else None
        try:
            if nw > 0:
                self._h_win[:nw] = torch.tensor([r[:2] for r in rows], dtype=torch.int64)
                nat.check(L.vad_ae_windows_forward_group(
                    pl.h, ring.data_ptr(), self.total_slots, cap, T, self._h_win.data_ptr(), nw,
                    self._table.data_ptr(), o["seq"].data_ptr(), o["err"].data_ptr(), o["mem"].data_ptr(),
                    o["score"].data_ptr(), nat.ptr(recon), stream))
        finally:
            self._copied.record(torch.cuda.current_stream(dev))
        # the pushed frames' latents, gathered through the destinations the device table already holds
        lat = ring_field(ring, self.total_slots, "lat").index_select(0, self._table[:F])
        outs, f0, r0 = [], 0, 0
        for s in range(S):
            _, widx0, n = stream_schedule(self.frames_seen[s], self.windows_emitted[s], ks[s], T, stride)
            r1 = r0 + n
            out = {
                "anomaly_scores": o["score"][r0:r1],
                "recon_errors": o["err"][r0:r1],
                "memory_scores": o["mem"][r0:r1],
                "sequence_features": o["seq"][r0:r1],
                "frame_features": lat[f0:f0 + ks[s]],
                "window_starts": (widx0 + torch.arange(n, dtype=torch.int64)) * stride,
            }
            if recon is not None:
                out["reconstructed"] = recon[r0:r1]
            outs.append(out)
            self.frames_seen[s] += ks[s]
            self.windows_emitted[s] = widx0 + n
            f0 += ks[s]
            r0 = r1
        return outs
