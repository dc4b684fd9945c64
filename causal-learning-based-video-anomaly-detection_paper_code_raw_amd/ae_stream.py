"""Scoring a live stream of frames with the memory autoencoder (VideoAutoEncoder, eval mode, forward only, fp32).

score_video (ae_video.py) needs the finished video in device memory and a frame cache as long as the video.  A stream
keeps the per-frame results in a ring of ``cap = window + max_push - 1`` slots instead -- frame g, counted from the
start of the stream, lives in slot ``g mod cap`` -- and scores, at every push, the windows the new frames complete
(vad_ae_frames_forward_ring / vad_ae_windows_forward_ring).  Every frame is still encoded once.  The window error
re-reads the window's raw frames, so the ring holds them too: lat [cap][64], gx [cap][256] and pix [cap][4096], 17.25
KB per slot.

Why cap slots are enough is stream.py's argument; the schedule is stream_util.stream_schedule.

Window w (frames ``w * stride .. w * stride + window - 1``) returns what score_video returns for it: the same stream
pushed in any chunking gives the results of score_video on the same frames.
"""
from __future__ import annotations

import torch

from . import _native as nat
from .ae_video import HW, LATENT
from .stream_util import _positive_int, check_push_u8, stream_schedule, u8_buffer

_RING_FIELDS = {"lat": (0, LATENT), "gx": (1, 4 * LATENT), "pix": (2, HW * HW)}


def ring_field(ring: torch.Tensor, cap: int, name: str) -> torch.Tensor:
    """View of one field of a ring: lat (cap, 64), gx (cap, 256), pix (cap, 4096)."""
    field, width = _RING_FIELDS[name]
    off = nat.lib().vad_ae_ring_offset(cap, field)
    if off < 0:
        nat.check(1)
    return ring[off:off + cap * width].view(cap, width)


def check_model(model):
    if model.training:
        raise ValueError("a stream runs in eval mode (running BatchNorm statistics): call model.eval()")


def check_push(model, frames, max_push) -> torch.Tensor:
    """The ValueErrors of AeStream.push, raised before any device work; returns the frames as (k, 1, 64, 64)."""
    check_model(model)
    if not isinstance(frames, torch.Tensor) or frames.dim() not in (4, 5):
        raise ValueError("push: frames of shape (k, 1, 64, 64) or (1, k, 1, 64, 64), got "
                         f"{tuple(getattr(frames, 'shape', ()))}")
    if frames.dim() == 5:
        if frames.shape[0] != 1:
            raise ValueError(f"push: one stream per call, got a batch of {frames.shape[0]}")
        frames = frames[0]
    if tuple(frames.shape[1:]) != (1, HW, HW):
        raise ValueError("push: frames of shape (k, 1, 64, 64) (the encoder's Linear(128*4*4) fixes 64x64 "
                         f"single-channel frames, cad1:151), got {tuple(frames.shape)}")
    k = frames.shape[0]
    if k < 1 or k > max_push:
        raise ValueError(f"push: between 1 and max_push = {max_push} frames per push, got {k}")
    return frames


class AeStream:
    """VideoAutoEncoder.open_stream's result.  All state is the ring and two counters; the model's (k, 1) plans are
    borrowed for the duration of a push only, so clip forwards, score_video calls and optimizer steps may run between
    pushes (a weight change makes later frames use the new weights).  A push changes no parameter, BatchNorm buffer or
    counter and leaves the memory ring and memory_ptr alone."""

    def __init__(self, model, window=16, stride=1, *, max_push=1, return_reconstructions=False):
        self.window = _positive_int("window", window)
        self.stride = _positive_int("stride", stride)
        self.max_push = _positive_int("max_push", max_push)
        # a push runs on a (max_push, 1) plan, and a plan holds at most as many clips as the memory ring has rows
        # (vad_ae_create: update_memory writes B rows of it)
        if self.max_push > model.memory_size:
            raise ValueError(f"open_stream: max_push must be at most {model.memory_size} (the clips one plan may "
                             f"hold), got {self.max_push}")
        check_model(model)
        self.model = model
        self.return_reconstructions = bool(return_reconstructions)
        self.cap = self.window + self.max_push - 1
        self._ring = None
        self._ingest = self._u8 = None  # push_u8's U8Ingest and its fp32 buffer of max_push frames
        self.frames_seen = 0
        self.windows_emitted = 0

    def reset(self):
        """Back to frame 0 and window 0; the ring is kept (nothing of it is read before it is written again)."""
        self.frames_seen = 0
        self.windows_emitted = 0

    def push(self, frames) -> dict:
        """frames: (k, 1, 64, 64) or (1, k, 1, 64, 64) on the device, 1 <= k <= max_push.  Encodes them and scores
        every window they complete; returns score_video's keys for exactly those windows (window_starts absolute;
        frame_features: the k pushed frames, a copy; empty tensors when no window completes)."""
        return self._push(check_push(self.model, frames, self.max_push))

    def push_u8(self, frames, color=None) -> dict:
        """frames: the next 1 <= k <= max_push frames as uint8 (k, Hs, Ws) or (k, 1, Hs, Ws) at any source size, on
        the device, in pinned host memory (read in place) or in pageable host memory.  One launch resizes them to
        64x64 as data.resize_u8 does and normalises them as the reference's dataset does, u8 / 255 clamped to
        0.001..0.999 (cad1:110-114), into a buffer the stream owns (data.U8Ingest); the rest is push: push_u8(u8)
        returns what push returns for the same frames converted on the host.  With color ("rgb", "bgr", "rgbx" or "bgrx") the frames are packed colour pixels, uint8
        (k, Hs, Ws, 3) or (k, Hs, Ws, 4), and the same launch takes their grey first (data.luma_u8, PIL's convert("L"))."""
        from .data import ingest_device
        check_model(self.model)
        x = check_push_u8(self.model, frames, self.max_push, color=color)
        dev = ingest_device(self.model, [x], "push_u8")
        ingest, buf = u8_buffer(self, dev, self.max_push, (HW, HW))
        return self._push(ingest.ingest(x, (HW, HW), 2, out=buf[:x.shape[0]], color=color))

    def _push(self, x) -> dict:
        """push's body: x (k, 1, 64, 64), checked."""
        T, stride, cap = self.window, self.stride, self.cap
        nat.require_hip(x)
        eng = self.model.engine()
        L = nat.lib()
        dev = eng.device
        x = x.to(torch.float32).contiguous()
        k = int(x.shape[0])
        stream = eng.stream()
        if self._ring is None:
            nfl = L.vad_ae_ring_floats(cap)
            if nfl < 0:
                nat.check(1)
            self._ring = torch.zeros(nfl, dtype=torch.float32, device=dev)
        ring = self._ring
        pl = eng.plan(k, 1)
        f0 = self.frames_seen
        nat.check(L.vad_ae_frames_forward_ring(pl.h, x.data_ptr(), cap, ring.data_ptr(), f0, stream))
        first, widx0, nw = stream_schedule(f0, self.windows_emitted, k, T, stride)
        o = dict(seq=torch.empty(nw, LATENT, device=dev), err=torch.empty(nw, device=dev),
                 mem=torch.empty(nw, device=dev), score=torch.empty(nw, device=dev))
        recon = torch.empty(nw, 1, HW, HW, device=dev) if self.return_reconstructions else None
        if nw > 0:
            nat.check(L.vad_ae_windows_forward_ring(
                pl.h, ring.data_ptr(), cap, T, stride, first, nw, o["seq"].data_ptr(), o["err"].data_ptr(),
                o["mem"].data_ptr(), o["score"].data_ptr(), nat.ptr(recon), stream))
        self.frames_seen = f0 + k
        self.windows_emitted = widx0 + nw
        # the pushed frames' slots s0 .. of the ring, in two runs where the chunk straddled the wrap
        s0 = f0 % cap
        n0 = min(k, cap - s0)
        lat = ring_field(ring, cap, "lat")
        out = {
            "anomaly_scores": o["score"],
            "recon_errors": o["err"],
            "memory_scores": o["mem"],
            "sequence_features": o["seq"],
            "frame_features": lat[s0:s0 + n0].clone() if n0 == k else torch.cat([lat[s0:], lat[:k - n0]]),
            "window_starts": (widx0 + torch.arange(nw, dtype=torch.int64)) * stride,
        }
        if recon is not None:
            out["reconstructed"] = recon
        return out
