"""Scoring a live stream of frames with CausalAnomalyDetector (eval mode, forward only, fp32).

score_video (video.py) needs the finished video in device memory and a frame cache as long as the video.  A stream
keeps the same per-frame results in a ring of ``cap = window + max_push - 1`` slots instead -- frame g, counted from
the start of the stream, lives in slot ``g mod cap`` -- and scores, at every push, the windows the new frames
complete (vad_cad_frames_forward_ring / vad_cad_windows_forward_ring).  Every frame's backbone still runs once.

Why cap slots are enough: window w covers frames ``w * stride .. w * stride + window - 1`` and is emitted by the push
that brings its last frame.  Before a push of k <= max_push frames, a frame older than the last ``window - 1`` can
only belong to windows that are complete, hence emitted; the push stores k new frames, so at most
``window - 1 + k <= cap`` frames are needed at once, and the frames it overwrites (g - cap for the new g) are older
than every one of them.  For the same reason the windows of one push span at most ``window + k - 1`` frames, which is
what vad_cad_windows_forward_ring asks of a batch.

Window w returns what ``model.eval(); model(clip_w, seed=seed, step=step, clip0=clip0 + w)`` returns, which is also
score_video's definition: the same stream pushed in any chunking gives the results of score_video on the same frames.

stream_schedule and the checks that no model enters are stream_util.py's, shared with the other three stream classes.
"""
from __future__ import annotations

import torch

from . import _native as nat
from .stream_util import _positive_int, check_frame_size, check_push_u8, stream_schedule, u8_buffer  # noqa: F401
from .video import MAX_DET, NUM_FACTORS, cache_field


def check_model(model):
    if model.training:
        raise ValueError("a stream runs in eval mode (running BatchNorm statistics, no dropout): call model.eval()")
    if getattr(model, "_compute_dtype", torch.float32) != torch.float32:
        raise ValueError("a stream computes in fp32 only: set_compute_dtype(torch.float32) first")


def check_push(model, frames, max_push, frame_size) -> torch.Tensor:
    """The ValueErrors of CadStream.push, raised before any device work; returns the frames as (k, 1, H, W).
    frame_size: (H, W) of the stream's first push, or None before it."""
    check_model(model)
    if not isinstance(frames, torch.Tensor) or frames.dim() not in (4, 5):
        raise ValueError("push: frames of shape (k, 1, H, W) or (1, k, 1, H, W), got "
                         f"{tuple(getattr(frames, 'shape', ()))}")
    if frames.dim() == 5:
        if frames.shape[0] != 1:
            raise ValueError(f"push: one stream per call, got a batch of {frames.shape[0]}")
        frames = frames[0]
    if frames.shape[1] != 1:
        raise ValueError("ResNetBackbone here takes single-channel frames (input_channels=1, cad:515)")
    k = frames.shape[0]
    if k < 1 or k > max_push:
        raise ValueError(f"push: between 1 and max_push = {max_push} frames per push, got {k}")
    if frame_size is not None and tuple(frames.shape[2:]) != tuple(frame_size):
        raise ValueError(f"push: frame size {tuple(frames.shape[2:])} differs from the stream's {tuple(frame_size)}")
    return frames


class CadStream:
    """CausalAnomalyDetector.open_stream's result.  All state is the ring and three counters; the model's plans are
    borrowed for the duration of a push only, so clip forwards, score_video calls and optimizer steps may run between
    pushes (a weight change makes later frames use the new weights)."""

    def __init__(self, model, window=16, stride=1, *, max_push=1, seed=0, step=0, clip0=0, frame_size=None):
        self.window = _positive_int("window", window)
        self.stride = _positive_int("stride", stride)
        self.max_push = _positive_int("max_push", max_push)
        check_model(model)
        self.model = model
        self.cap = self.window + self.max_push - 1
        self.seed, self.step, self.clip0 = int(seed), int(step), int(clip0)
        # (H, W) of the frames the model sees: given, or fixed by the first push (a u8 push: its source size)
        self.frame_size = check_frame_size(frame_size)
        self._ring = None
        self._ingest = self._u8 = None  # push_u8's U8Ingest and its fp32 buffer of max_push frames
        self.frames_seen = 0
        self.windows_emitted = 0

    def reset(self):
        """Back to frame 0 and window 0; the ring is kept (nothing of it is read before it is written again)."""
        self.frames_seen = 0
        self.windows_emitted = 0

    def push(self, frames) -> dict:
        """frames: (k, 1, H, W) or (1, k, 1, H, W) on the device, 1 <= k <= max_push.  Runs the per-frame stage on
        them and every window they complete; returns score_video's keys for exactly those windows (window_starts
        absolute; detections: the k pushed frames; empty tensors when no window completes)."""
        return self._push(check_push(self.model, frames, self.max_push, self.frame_size))

    def push_u8(self, frames, color=None) -> dict:
        """frames: the next 1 <= k <= max_push frames as uint8 (k, Hs, Ws) or (k, 1, Hs, Ws) at any source size, on
        the device, in pinned host memory (read in place) or in pageable host memory.  One launch resizes them to the
        stream's frame size as data.resize_u8 does and normalises them as (u8 - 0.5) / 0.5 into a buffer the stream
        owns (data.U8Ingest); the rest is push: push_u8(u8) returns what push returns for the same frames converted
        on the host.  Without frame_size the first push fixes it to the source size.  With color ("rgb", "bgr", "rgbx" or "bgrx") the frames are packed colour pixels, uint8
        (k, Hs, Ws, 3) or (k, Hs, Ws, 4), and the same launch takes their grey first (data.luma_u8, PIL's convert("L"))."""
        from .data import ingest_device
        check_model(self.model)
        x = check_push_u8(self.model, frames, self.max_push, color=color)
        dev = ingest_device(self.model, [x], "push_u8")
        size = self.frame_size or tuple(x.shape[1:3])
        ingest, buf = u8_buffer(self, dev, self.max_push, size)
        return self._push(ingest.ingest(x, size, 0, out=buf[:x.shape[0]], color=color))

    def _push(self, x) -> dict:
        """push's body: x (k, 1, H, W), checked."""
        model, T, stride, cap = self.model, self.window, self.stride, self.cap
        eng = model.engine()
        nat.require_hip(x)
        L = nat.lib()
        dev = eng.device
        x = x.contiguous().float()
        k, _, H, W = x.shape
        stream = nat.stream_of(dev)
        if self._ring is None:
            nfl = L.vad_cad_frame_cache_floats(cap)
            if nfl < 0:
                nat.check(1)
            self._ring = torch.zeros(nfl, dtype=torch.float32, device=dev)
            self.frame_size = (H, W)
        ring = self._ring
        # a forward armed for another input must not outlive this call (CadEngine.input_ready)
        armed, eng._armed = getattr(eng, "_armed", None), None
        if armed is not None:
            nat.check(L.vad_cad_set_option(armed.h, b"input_armed", 0))
        # (the plan's activations are overwritten: a backward still pending on an earlier forward must not read them)
        eng.generation += 1
        pl = eng.plan(k, 1, H, W)
        eng._set_stem_grad(pl)
        eng._check_images(pl)
        f0 = self.frames_seen
        nat.check(L.vad_cad_frames_forward_ring(pl.h, x.data_ptr(), cap, ring.data_ptr(), f0, stream))
        first, widx0, nw = stream_schedule(f0, self.windows_emitted, k, T, stride)
        o = dict(final=torch.empty(nw, device=dev), probs=torch.empty(nw, 2, device=dev),
                 causal=torch.empty(nw, device=dev), kl=torch.empty(nw, device=dev),
                 z=torch.empty(nw, MAX_DET, NUM_FACTORS, device=dev),
                 adj=torch.empty(nw, NUM_FACTORS, NUM_FACTORS, device=dev),
                 nmax=torch.empty(nw, dtype=torch.int32, device=dev))
        if nw > 0:
            nat.check(L.vad_cad_windows_forward_ring(
                pl.h, ring.data_ptr(), cap, T, stride, first, widx0, nw, self.seed & ((1 << 64) - 1), self.step,
                self.clip0, o["final"].data_ptr(), o["probs"].data_ptr(), o["causal"].data_ptr(), o["kl"].data_ptr(),
                o["z"].data_ptr(), o["adj"].data_ptr(), o["nmax"].data_ptr(), stream))
        self.frames_seen = f0 + k
        self.windows_emitted = widx0 + nw
        # the pushed frames' slots s0 .. of the ring, in two runs where the chunk straddled the wrap
        s0 = f0 % cap
        n0 = min(k, cap - s0)

        def pushed(name):
            v = cache_field(ring, cap, name)
            return v[s0:s0 + n0].clone() if n0 == k else torch.cat([v[s0:], v[:k - n0]])

        boxes = pushed("boxes")
        cnt = pushed("counts").tolist()
        nm = o["nmax"].tolist()
        return {
            "anomaly_scores": o["final"],
            "direct_predictions": o["probs"],
            "causal_anomaly_scores": o["causal"],
            "kl_losses": o["kl"],
            "adjacency_matrices": o["adj"],
            "causal_factors": [o["z"][w, :nm[w]] for w in range(nw)],
            "detections": [boxes[f, :cnt[f]] for f in range(k)],
            "window_starts": (widx0 + torch.arange(nw, dtype=torch.int64)) * stride,
        }
