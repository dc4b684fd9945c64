"""Scoring video and live streams with the three 3-D clip models -- a2.CausalAnomalyDetector,
mc.SimpleVideoAnomalyDetector and bbox.CausalAnomalyDetector -- without building clips.

A clip model's first conv can read window b of a frame-major planar buffer in place (csrc/common.h WinSrc): frame
``first + b * stride + t``, modulo ``ring`` for a ring of raw frames.  Two things are built on that here:

  * ``score_video`` (a2, mc; bbox has its own): the windows of a finished video, ``batch`` per call;
  * ``ClipStream`` (``model.open_stream``): a ring of ``cap = window + max_push - 1`` raw frames in one device
    allocation -- frame g of the stream lives in slot ``g mod cap`` -- and, at every push, one windows call for exactly
    the windows the new frames complete (stream_util.stream_schedule; why cap slots are enough is stream.py's argument:
    a window completed by a push started at most window - 1 frames before it).

The three models differ in the windows call and the output keys only (their engines' ``windows_forward``,
``window_outputs`` and ``WINDOW_KEYS``).  No conv work is shared between overlapping windows: temporal padding, pooling
and striding are placed relative to each window's first frame, so from the second layer on a frame's activations
depend on where its window starts.  What the in-place form saves is the copy of every window into a clip.

A windows call runs the clip path's kernels on the same number of clips, so a batch of windows gives what
``model(clips)`` gives for those windows gathered into one batch (a2, a single window: the clip twice, row 0 -- its plans
hold at least two clips).  As for ``model(clips)``, the batch is part of the result to the last bit where a kernel is
chosen by it: bbox's head GEMMs by the row count (up to 8, up to 16, more), a2's conv3d_2 / conv3d_3 GEMMs the split of
their reduction by the number of output tiles; minicausal has no such choice.  A stream therefore equals score_video
bit for bit when score_video's ``batch`` keeps it in the kernels a push runs (``batch=8`` does for pushes of up to 8
windows of small frames), and to rounding otherwise.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import _native as nat
from .stream_util import _positive_int, check_frame_size, check_push_u8, stream_schedule


class _Kind(NamedTuple):
    channels: object   # model -> the channel count of its frames
    min_window: int    # the shortest clip the plan accepts (vad_*_create)
    min_hw: int        # the smallest frame side
    why: str


KINDS = {
    "a2": _Kind(lambda m: 3, 1, 4, "vad_a2_create: T >= 1, H, W >= 4"),
    "mc": _Kind(lambda m: m.features[0].in_channels, 4, 8, "the three MaxPool3d stages: T >= 4, H, W >= 8"),
    "bbox": _Kind(lambda m: 3, 2, 2, "MaxPool3d(2): T, H, W >= 2"),
}


def _integer(what, name, v, least):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or int(v) != v or v < least:
        raise ValueError(f"{what}: {name} must be an integer >= {least}, got {v!r}")
    return int(v)


def check_frames(kind, model, frames, what) -> torch.Tensor:
    """The ValueErrors every fp32 frame source raises, before any device work: eval mode, (n, C, H, W) floating point
    with the model's channel count and at least the smallest frame its plan accepts."""
    k = KINDS[kind]
    if model.training:
        raise ValueError(f"{what} runs in eval mode (no dropout, BatchNorm on the running statistics): call model.eval()")
    C = k.channels(model)
    if not isinstance(frames, torch.Tensor) or frames.dim() != 4 or frames.shape[1] != C:
        raise ValueError(f"{what}: frames of shape (N, {C}, H, W), planar, got "
                         f"{tuple(getattr(frames, 'shape', ())) or type(frames).__name__}")
    if not frames.is_floating_point():
        raise ValueError(f"{what}: frames must be floating point (uint8 frames go through data.ingest_u8 or push_u8), "
                         f"got {frames.dtype}")
    if min(frames.shape[2:]) < k.min_hw:
        raise ValueError(f"{what}: frames of at least {k.min_hw} x {k.min_hw} pixels ({k.why}), got "
                         f"{tuple(frames.shape)}")
    return frames


def check_score_video(kind, model, frames, window, stride, batch) -> torch.Tensor:
    """The ValueErrors of a2's and mc's score_video, raised before any device work; returns the frames."""
    x = check_frames(kind, model, frames, "score_video")
    _integer("score_video", "window", window, KINDS[kind].min_window)
    _integer("score_video", "stride", stride, 1)
    _integer("score_video", "batch", batch, 1)
    if x.shape[0] < window:
        raise ValueError(f"score_video: the video has {x.shape[0]} frames, fewer than one window of {window}")
    return x


def window_starts(n_frames: int, window: int, stride: int) -> torch.Tensor:
    """The first frame of every full window of a video of n_frames frames (int64, host)."""
    return torch.arange((n_frames - window) // stride + 1 if n_frames >= window else 0, dtype=torch.int64) * stride


def score_video(eng, x, window, stride, batch) -> dict:
    """x (N, C, H, W) fp32 contiguous on eng's device, checked: its windows, ``batch`` per windows call."""
    starts = window_starts(x.shape[0], window, stride)
    Wn = len(starts)
    out = eng.window_outputs(Wn)
    for w0 in range(0, Wn, batch):
        eng.windows_forward(x, w0 * stride, stride, 0, min(batch, Wn - w0), window, min(batch, Wn),
                            tuple(o[w0:] for o in out))
    return {**dict(zip(eng.WINDOW_KEYS, out)), "window_starts": starts}


def ring_slots(window: int, max_push: int) -> int:
    return window + max_push - 1


class ClipStream:
    """``open_stream``'s result on a clip model.  All state is the ring of raw frames and two counters; the model's
    scoring plans are borrowed for the duration of a push, so clip forwards, train steps and score_video calls may run
    between pushes (a weight change makes later windows use the new weights), and two streams on one model share the
    plans but not the rings.  A push changes no parameter, buffer or counter of the model."""

    def __init__(self, model, kind, window, stride=1, *, max_push=1, frame_size=None):
        k = KINDS[kind]
        self.window = _integer("open_stream", "window", window, k.min_window)
        self.stride = _positive_int("stride", stride)
        self.max_push = _positive_int("max_push", max_push)
        self.frame_size = check_frame_size(frame_size)
        if self.frame_size is not None and min(self.frame_size) < k.min_hw:
            raise ValueError(f"open_stream: frame_size of at least {k.min_hw} x {k.min_hw} ({k.why}), got {frame_size!r}")
        if model.training:
            raise ValueError("a stream runs in eval mode (no dropout, BatchNorm on the running statistics): call "
                             "model.eval()")
        self.model, self.kind = model, kind
        self.channels = k.channels(model)
        self.cap = ring_slots(self.window, self.max_push)
        self.max_windows = -(-self.max_push // self.stride)  # a push of k frames completes at most ceil(k / stride)
        self._ring = None    # (cap, C, H, W) fp32
        self._ingest = self._u8 = None  # push_u8's U8Ingest, and its buffer where a ring slot is not 16-byte aligned
        self.frames_seen = 0
        self.windows_emitted = 0

    def reset(self):
        """Back to frame 0 and window 0; the ring is kept (nothing of it is read before it is written again)."""
        self.frames_seen = 0
        self.windows_emitted = 0

    # ------------------------------------------------------------------ checks (no device work)
    def _check_size(self, size, what):
        if self.frame_size is not None and tuple(size) != self.frame_size:
            raise ValueError(f"{what}: frames of {tuple(size)}, but the stream's frames are {self.frame_size}")

    def _check_push(self, frames) -> torch.Tensor:
        x = check_frames(self.kind, self.model, frames, "push")
        if x.shape[0] < 1 or x.shape[0] > self.max_push:
            raise ValueError(f"push: between 1 and max_push = {self.max_push} frames per push, got {x.shape[0]}")
        self._check_size(x.shape[2:], "push")
        return x

    # ------------------------------------------------------------------ the ring
    def _slots(self, k):
        """The runs of ring slots the next k frames go to: [(slot0, n, frame0 of the push)], two where they straddle
        the ring's end."""
        s0 = self.frames_seen % self.cap
        n0 = min(k, self.cap - s0)
        return [(s0, n0, 0)] + ([(0, k - n0, n0)] if n0 < k else [])

    def _ring_on(self, dev, size):
        if self._ring is None:
            self.frame_size = tuple(int(v) for v in size)
            self._ring = torch.zeros(self.cap, self.channels, *self.frame_size, dtype=torch.float32, device=dev)
        elif self._ring.device != dev:
            raise ValueError(f"push: frames on {dev}, but the stream's ring is on {self._ring.device}")
        return self._ring

    def push(self, frames) -> dict:
        """frames: the next 1 <= k <= max_push frames (k, C, H, W), floating point, on the device.  Copies them into
        their ring slots and scores exactly the windows they complete, straight from the ring; returns score_video's
        keys for those windows (window_starts counted from the stream's first frame; empty tensors, and no launch,
        when no window completes)."""
        x = self._check_push(frames)
        nat.require_hip(x)
        x = x.float().contiguous()
        ring = self._ring_on(x.device, x.shape[2:])
        for s0, n, f0 in self._slots(x.shape[0]):
            ring[s0:s0 + n].copy_(x[f0:f0 + n])
        return self._score(x.shape[0])

    def push_u8(self, frames, color=None) -> dict:
        """frames: the next 1 <= k <= max_push frames as uint8 at any source size, on the device, in pinned host
        memory (read in place) or in pageable host memory.  A 1-channel model takes grey frames (k, Hs, Ws) or
        (k, 1, Hs, Ws), or with ``color`` packed colour frames (k, Hs, Ws, 3 or 4) whose luma it takes; a 3-channel
        model needs ``color`` ("rgb", "bgr", "rgbx", "bgrx") and gets planar RGB.  One data.U8Ingest launch resizes
        them to the stream's frame_size (open_stream's argument, or an earlier push's size) as data.resize_u8 does and
        divides by 255 (mode 1), straight into the ring slots -- two launches where the frames straddle the ring's
        end; through a buffer of max_push frames and a copy where a slot is not 16-byte aligned (C * H * W no
        multiple of 4), which the ingest's stores need.  Returns exactly what push returns for
        ``data.ingest_u8(frames, frame_size, 1, color=color, planes=C)``."""
        from .data import U8Ingest, ingest_device
        if self.model.training:
            raise ValueError("push_u8 runs in eval mode (no dropout, BatchNorm on the running statistics): call "
                             "model.eval()")
        C = self.channels
        if C not in (1, 3):
            raise ValueError(f"push_u8: grey or RGB frames only, but the model reads {C} channels")
        if C == 3 and color is None:
            raise ValueError("push_u8: the model reads planar RGB: name the frames' colour format (color=\"rgb\", "
                             "\"bgr\", \"rgbx\" or \"bgrx\")")
        x = check_push_u8(self.model, frames, self.max_push, color=color)
        if self.frame_size is None:
            raise ValueError("push_u8: the stream does not know its frame size yet: pass frame_size=(H, W) to "
                             "open_stream")
        dev = ingest_device(self.model, [x], "push_u8")
        ring = self._ring_on(dev, self.frame_size)
        if self._ingest is None:
            self._ingest = U8Ingest(dev)
        k = x.shape[0]
        if ring[0].numel() % 4 == 0:
            for s0, n, f0 in self._slots(k):
                self._ingest.ingest(x[f0:f0 + n], self.frame_size, 1, out=ring[s0:s0 + n], color=color, planes=C)
        else:
            if self._u8 is None:
                self._u8 = torch.empty(self.max_push, *ring.shape[1:], dtype=torch.float32, device=dev)
            buf = self._ingest.ingest(x, self.frame_size, 1, out=self._u8[:k], color=color, planes=C)
            for s0, n, f0 in self._slots(k):
                ring[s0:s0 + n].copy_(buf[f0:f0 + n])
        return self._score(k)

    def _score(self, k) -> dict:
        """The k frames after frames_seen are in their slots: score the windows they complete."""
        eng = self.model.scoring_engine(self._ring.device)
        first, widx0, nw = stream_schedule(self.frames_seen, self.windows_emitted, k, self.window, self.stride)
        out = eng.window_outputs(nw)
        if nw > 0:
            eng.windows_forward(self._ring, first % self.cap, self.stride, self.cap, nw, self.window, self.max_windows,
                                out)
        self.frames_seen += k
        self.windows_emitted = widx0 + nw
        return {**dict(zip(eng.WINDOW_KEYS, out)),
                "window_starts": (widx0 + torch.arange(nw, dtype=torch.int64)) * self.stride}
