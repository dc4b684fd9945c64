"""Scoring many live streams with the memory autoencoder in shared launches (VideoAutoEncoder, eval mode, forward
only, fp32).

One AeStream per camera costs one launch-bound push per camera.  In eval mode every per-frame result depends on its
frame alone and every per-window result on its window alone, so a group runs the frames of all its streams through one
per-frame pass and all the windows they complete through one per-window pass (vad_ae_frames_forward_group /
vad_ae_windows_forward_group).

Memory is one ring allocation of ``num_streams * cap`` slots, cap = window + max_push - 1 (ae_stream.py's three arrays
lat, gx and pix over that many slots): ring s occupies slots ``s * cap .. (s + 1) * cap - 1`` of each array and frame
g of stream s lives in slot ``s * cap + g mod cap``; stream.py's argument for why cap slots suffice holds per stream.
Where a frame goes and which slots a window reads are tables built on the host (stream_util.group_schedule, whose
key column is not used here, held in a stream_util.GroupTables), validated by the library (csrc/group_table.h) and
copied to the device once per stage.

The ``F = sum of k_s`` frames of a push are zero-padded to the next power of two (at most num_streams * max_push), the
padding frames being stored nowhere, so a group creates at most ``ceil(log2(num_streams * max_push)) + 1`` plans
instead of one per distinct F (stream_util.padded_frames).

Stream s returns what ``model.open_stream(window, stride, max_push=max_push, return_reconstructions=...)`` returns
for the same history of frames.
"""
from __future__ import annotations

import torch

from . import _native as nat
from .ae_stream import check_model, ring_field
from .ae_video import HW, LATENT
from .stream_util import (GroupTables, _positive_int, gather_padded, group_schedule, padded_frames,  # noqa: F401
                          per_stream, stream_schedule, u8_buffer, walk_group_frames, walk_group_frames_u8)


def check_group_push(model, frames, num_streams, max_push):
    """The ValueErrors of AeStreamGroup.push, raised before any device work.  Returns (chunks, ks): per stream the
    frames as (k_s, 1, 64, 64), or None where k_s = 0."""
    check_model(model)

    def check_one(s, x):
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or tuple(x.shape[1:]) != (1, HW, HW):
            raise ValueError(f"push: stream {s}: frames of shape (k, 1, 64, 64) or None (the encoder's "
                             "Linear(128*4*4) fixes 64x64 single-channel frames, cad1:151), got "
                             f"{tuple(getattr(x, 'shape', ()))}")
        return x

    return walk_group_frames(frames, num_streams, max_push, "push", check_one, "frames (k, 1, 64, 64) or None")


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
        if nfl < 0:
            nat.check(1)
        self._ring = torch.zeros(nfl, dtype=torch.float32, device=dev)
        # the device table and the pinned host tables the library copies from (stream_util.GroupTables).
        # Unlike CadStreamGroup.push, a push here ends with no host read, so it may return -- and the next push begin
        # -- before the device has copied the tables: _copied is recorded on the stream behind the last table copy of
        # a push, and the next push waits for it before it writes the host tables again (it has normally passed)
        self._tables = GroupTables(L.vad_ae_group_table_bytes, self.max_frames, 2, dev)
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
        return self._push(gather_padded(live, F, padded_frames(F, self.max_frames), (1, HW, HW)), ks)

    def push_u8(self, frames, color=None) -> list:
        """frames: a sequence of num_streams entries, entry s the next 0 <= k_s <= max_push frames of camera s as uint8
        (k_s, Hs, Ws) or (k_s, 1, Hs, Ws), or None; cameras may differ in source size and in where their frames lie
        (device, pinned host memory read in place, pageable host memory).  One table-form launch resizes every frame
        to 64x64 as data.resize_u8 does, normalises it as u8 / 255 clamped to 0.001..0.999 (cad1:110-114) and writes
        the zero padding, into a buffer the group owns (data.U8Ingest.table); the rest is push: push_u8 returns what
        push returns for the same frames converted on the host.  With color ("rgb", "bgr", "rgbx" or "bgrx") every camera brings packed colour pixels,
        uint8 (k_s, Hs, Ws, 3) or (k_s, Hs, Ws, 4) -- one format for the whole call -- and the same launch takes their
        grey first (data.luma_u8, PIL's convert("L"))."""
        from .data import ingest_device
        check_model(self.model)
        chunks, ks = walk_group_frames_u8(frames, self.num_streams, self.max_push, color)
        live = [x for x in chunks if x is not None]
        dev = ingest_device(self.model, live, "push_u8")
        ingest, buf = u8_buffer(self, dev, self.max_frames, (HW, HW))
        P = padded_frames(sum(ks), self.max_frames)
        x = ingest.table(live, P, (HW, HW), 2, out=buf[:P], capacity=self.max_frames, color=color)
        return self._push(x, ks)

    def _push(self, x, ks) -> list:
        """push's body: x (P, 1, 64, 64), the sum(ks) frames in stream order, then zeros."""
        T, stride, cap = self.window, self.stride, self.cap
        eng = self.model.engine()
        L = nat.lib()
        dev = eng.device
        stream = eng.stream()
        if self._ring is None:
            self._allocate(L, dev)
        ring, tables = self._ring, self._tables
        F, P = sum(ks), x.shape[0]
        dst, rows = group_schedule(self.frames_seen, self.windows_emitted, ks, T, stride, cap=cap)
        nw = len(rows)
        self._copied.synchronize()  # (see _allocate: the device has the tables of the push before)
        tables.fill_dst(dst, P)
        pl = eng.plan(P, 1)
        nat.check(L.vad_ae_frames_forward_group(pl.h, x.data_ptr(), self.total_slots, ring.data_ptr(),
                                                tables.h_dst.data_ptr(), tables.dev.data_ptr(), stream))
        o = dict(seq=torch.empty(nw, LATENT, device=dev), err=torch.empty(nw, device=dev),
                 mem=torch.empty(nw, device=dev), score=torch.empty(nw, device=dev))
        recon = torch.empty(nw, 1, HW, HW, device=dev) if self.return_reconstructions else None
        try:
            if nw > 0:
                tables.fill_windows([r[:2] for r in rows])
                nat.check(L.vad_ae_windows_forward_group(
                    pl.h, ring.data_ptr(), self.total_slots, cap, T, tables.h_win.data_ptr(), nw,
                    tables.dev.data_ptr(), o["seq"].data_ptr(), o["err"].data_ptr(), o["mem"].data_ptr(),
                    o["score"].data_ptr(), nat.ptr(recon), stream))
        finally:
            self._copied.record(torch.cuda.current_stream(dev))
        # the pushed frames' latents, gathered through the destinations the device table already holds
        lat = ring_field(ring, self.total_slots, "lat").index_select(0, tables.dev[:F])
        outs = []
        for s, f0, f1, r0, r1, widx0, n in per_stream(self.frames_seen, self.windows_emitted, ks, T, stride):
            out = {
                "anomaly_scores": o["score"][r0:r1],
                "recon_errors": o["err"][r0:r1],
                "memory_scores": o["mem"][r0:r1],
                "sequence_features": o["seq"][r0:r1],
                "frame_features": lat[f0:f1],
                "window_starts": (widx0 + torch.arange(n, dtype=torch.int64)) * stride,
            }
            if recon is not None:
                out["reconstructed"] = recon[r0:r1]
            outs.append(out)
        return outs
