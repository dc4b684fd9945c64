"""Scoring many live streams of one frame size with a 3-D clip model -- a2.CausalAnomalyDetector,
mc.SimpleVideoAnomalyDetector or bbox.CausalAnomalyDetector -- in one windows call per push (eval mode,
forward only, fp32).

One ClipStream per camera costs one launch-bound chain of launches per camera.  A clip model caches nothing per frame,
so a group is a ring of raw frames per camera plus a table: the first conv finds window b of the batch through row b
of a device table, (base, first) -- slot ``base + (first + t) mod cap`` of one allocation (csrc/common.h WinSrc, group
form) -- and everything behind the first conv is batched over windows already.

Memory is one allocation ``(num_streams * cap, C, H, W)``, cap = window + max_push - 1: ring s occupies slots
``s * cap .. (s + 1) * cap - 1`` and frame g of stream s lives in slot ``s * cap + g mod cap``; stream.py's argument
for why cap slots suffice holds per stream.  Where a frame goes and which slots a window reads come from
stream_util.group_schedule (its key column is not used); the rows are validated by the library (csrc/group_table.h)
and copied to the device once per push.

A push runs the clip path's kernels on the windows of all its streams as one batch, so its outputs, concatenated in
stream order, are what ``model(clips)`` gives for those windows gathered into one batch in that order (a2, a single
window: the clip twice, row 0).  Against one ClipStream per camera the batch differs, which is part of the result to
the last bit where a kernel is chosen by it (clip_stream.py): minicausal is equal bit for bit, a2 and bbox wherever the
group's batch and the lone stream's stay in the same kernels, and to rounding otherwise.
"""
from __future__ import annotations

import torch

from . import _native as nat
from .clip_stream import KINDS, _integer, check_frames, ring_slots
from .stream_util import (_positive_int, check_frame_size, group_schedule, per_stream, walk_group_frames,
                          walk_group_frames_u8)

# the most clips one scoring plan holds (vad_a2_create, vad_mc_create); bbox's plans have no such limit
PLAN_LIMIT = {"a2": ("A2_MAXB", 256), "mc": ("MC_MAXB", 1024)}


def _check_eval(model, what):
    if model.training:
        raise ValueError(f"{what} runs in eval mode (no dropout, BatchNorm on the running statistics): call "
                         "model.eval()")


def check_group_push(kind, model, frames, num_streams, max_push, frame_size):
    """The ValueErrors of ClipStreamGroup.push, raised before any device work.  Returns (chunks, ks, (H, W)): per
    stream the frames as (k_s, C, H, W), or None where k_s = 0."""
    _check_eval(model, "push")
    size = [frame_size]  # the group's, or that of the first frames seen

    def check_one(s, x):
        x = check_frames(kind, model, x, f"push: stream {s}")
        if 0 < x.shape[0] <= max_push:  # (more than max_push frames: the walk's error comes first)
            if size[0] is None:
                size[0] = tuple(int(v) for v in x.shape[2:])
            elif tuple(x.shape[2:]) != tuple(size[0]):
                raise ValueError(f"push: stream {s}: frame size {tuple(x.shape[2:])} differs from the group's "
                                 f"{tuple(size[0])}")
        return x

    C = KINDS[kind].channels(model)
    chunks, ks = walk_group_frames(frames, num_streams, max_push, "push", check_one, f"frames (k, {C}, H, W) or None")
    return chunks, ks, size[0]


def window_rows(frames_seen, windows_emitted, ks, window, stride, cap):
    """(dst, rows) of one push: group_schedule's destinations and the (base, first) columns of its window rows."""
    dst, rows = group_schedule(frames_seen, windows_emitted, ks, window, stride, cap=cap)
    return dst, [r[:2] for r in rows]


class _Tables:
    """The tables of a ClipStreamGroup: dev, the device table of vad_win_group_table_bytes(max_windows) bytes, and the
    pinned host images h_win (max_windows rows of (base, first)) and h_dst (the ring slot of every pushed frame)."""

    def __init__(self, max_frames, max_windows, dev):
        nb = nat.lib().vad_win_group_table_bytes(max_windows)
        if nb < 0:
            nat.check(1)
        self.dev = torch.zeros(nb // 8, dtype=torch.int64, device=dev)
        self.h_win = torch.empty(max_windows, 2, dtype=torch.int64).pin_memory()
        self.h_dst = torch.empty(max_frames, dtype=torch.int64).pin_memory()


class ClipStreamGroup:
    """``open_stream_group``'s result on a clip model: num_streams rings in one allocation, two counters per stream,
    one device table and its pinned host images.  As with ClipStream the model's scoring plans are borrowed for the
    duration of a push only, and a push changes no parameter, buffer or counter of the model."""

    def __init__(self, model, kind, num_streams, window, stride=1, *, max_push=1, frame_size=None):
        k = KINDS[kind]
        self.num_streams = _positive_int("num_streams", num_streams)
        self.window = _integer("open_stream_group", "window", window, k.min_window)
        self.stride = _positive_int("stride", stride)
        self.max_push = _positive_int("max_push", max_push)
        self.frame_size = check_frame_size(frame_size, "open_stream_group")
        if self.frame_size is not None and min(self.frame_size) < k.min_hw:
            raise ValueError(f"open_stream_group: frame_size of at least {k.min_hw} x {k.min_hw} ({k.why}), got "
                             f"{frame_size!r}")
        _check_eval(model, "a stream group")
        self.model, self.kind = model, kind
        self.channels = k.channels(model)
        self.cap = ring_slots(self.window, self.max_push)
        self.total_slots = self.num_streams * self.cap
        self.max_frames = self.num_streams * self.max_push
        # a push of k frames completes at most ceil(k / stride) windows of its stream; one plan holds them all
        self.max_windows = self.num_streams * -(-self.max_push // self.stride)
        if kind in PLAN_LIMIT and self.max_windows > PLAN_LIMIT[kind][1]:
            name, limit = PLAN_LIMIT[kind]
            raise ValueError(f"open_stream_group: num_streams * ceil(max_push / stride) must be at most {limit} (the "
                             f"clips one plan may hold, {name}), got {self.num_streams} * "
                             f"{self.max_windows // self.num_streams} = {self.max_windows}")
        self._ring = None    # (total_slots, C, H, W) fp32
        self._ingest = self._u8 = None  # push_u8's U8Ingest and its fp32 buffer of max_frames frames
        self.frames_seen = [0] * self.num_streams
        self.windows_emitted = [0] * self.num_streams

    def reset(self, s=None):
        """Stream s, or every stream, back to frame 0 and window 0; the rings are kept (nothing of them is read before
        it is written again)."""
        for i in range(self.num_streams) if s is None else [s]:
            self.frames_seen[i] = 0
            self.windows_emitted[i] = 0

    def _allocate(self, dev, size):
        self.frame_size = tuple(int(v) for v in size)
        self._ring = torch.zeros(self.total_slots, self.channels, *self.frame_size, dtype=torch.float32, device=dev)
        # A push ends with no host read, so it may return -- and the next push begin -- before the device has copied
        # the pinned host tables: _copied is recorded on the stream behind the last copy of a push, and the next push
        # waits for it before it writes h_dst or h_win again (it has normally passed).  The event holds the order, as
        # in AeStreamGroup; CadStreamGroup's argument (a host read at the end of every push) does not apply here.
        self._tables = _Tables(self.max_frames, self.max_windows, dev)
        self._copied = torch.cuda.Event()

    def push(self, frames) -> list:
        """frames: a sequence of num_streams entries, entry s the next 0 <= k_s <= max_push frames of stream s as
        (k_s, C, H, W), floating point, on the device, or None.  Returns one ClipStream.push dict per stream: the
        windows that stream's frames complete, window_starts counted from its first frame; empty tensors where it
        completed none.  A push in which no stream completes a window makes no library call."""
        chunks, ks, size = check_group_push(self.kind, self.model, frames, self.num_streams, self.max_push,
                                            self.frame_size)
        live = [x for x in chunks if x is not None]
        for x in live:
            nat.require_hip(x)
        if self._ring is not None and live[0].device != self._ring.device:
            raise ValueError(f"push: frames on {live[0].device}, but the group's rings are on {self._ring.device}")
        return self._push(torch.cat([x.float() for x in live]), ks, size)

    def push_u8(self, frames, color=None) -> list:
        """frames: a sequence of num_streams entries, entry s the next 0 <= k_s <= max_push frames of camera s as
        uint8, or None; cameras may differ in source size and in where their frames lie (device, pinned host memory
        read in place, pageable host memory).  A 1-channel model takes grey frames (k_s, Hs, Ws) or (k_s, 1, Hs, Ws),
        or with ``color`` packed colour frames (k_s, Hs, Ws, 3 or 4) whose luma it takes; a 3-channel model needs
        ``color`` ("rgb", "bgr", "rgbx", "bgrx") and gets planar RGB -- one format for the whole call.  One table-form
        launch (data.U8Ingest.table) resizes every frame to the group's frame_size (open_stream_group's argument, or an
        earlier push's size) as data.resize_u8 does and divides by 255 (mode 1), into a buffer the group owns; the
        rest is push: push_u8 returns exactly what push returns for
        ``data.ingest_u8(frames_s, frame_size, 1, color=color, planes=C)`` of every camera."""
        from .data import U8Ingest, ingest_device
        _check_eval(self.model, "push_u8")
        C = self.channels
        if C not in (1, 3):
            raise ValueError(f"push_u8: grey or RGB frames only, but the model reads {C} channels")
        if C == 3 and color is None:
            raise ValueError("push_u8: the model reads planar RGB: name the frames' colour format (color=\"rgb\", "
                             "\"bgr\", \"rgbx\" or \"bgrx\")")
        chunks, ks = walk_group_frames_u8(frames, self.num_streams, self.max_push, color)
        if self.frame_size is None:
            raise ValueError("push_u8: the group does not know its frame size yet: pass frame_size=(H, W) to "
                             "open_stream_group")
        live = [x for x in chunks if x is not None]
        dev = ingest_device(self.model, live, "push_u8")
        if self._ingest is None:
            self._ingest = U8Ingest(dev)
            self._u8 = torch.empty(self.max_frames, C, *self.frame_size, dtype=torch.float32, device=dev)
        F = sum(ks)
        x = self._ingest.table(live, F, self.frame_size, 1, out=self._u8[:F], capacity=self.max_frames, color=color,
                               planes=C)
        return self._push(x, ks, self.frame_size)

    def _push(self, x, ks, size) -> list:
        """push's body: x (F, C, H, W) fp32 on the device, the sum(ks) frames in stream order."""
        T, stride, cap = self.window, self.stride, self.cap
        dev = x.device
        eng = self.model.scoring_engine(dev)
        if self._ring is None:
            self._allocate(dev, size)
        ring, tables = self._ring, self._tables
        F = sum(ks)
        dst, rows = window_rows(self.frames_seen, self.windows_emitted, ks, T, stride, cap)
        nw = len(rows)
        self._copied.synchronize()  # (see _allocate: the device has the tables of the push before)
        tables.h_dst[:F] = torch.tensor(dst, dtype=torch.int64)
        ring.index_copy_(0, tables.h_dst[:F].to(dev, non_blocking=True), x)
        out = eng.window_outputs(nw)
        try:
            if nw > 0:
                tables.h_win[:nw] = torch.tensor(rows, dtype=torch.int64)
                eng.windows_forward_group(ring, cap, tables.h_win, nw, tables.dev, T, self.max_windows, out)
        finally:
            self._copied.record(torch.cuda.current_stream(dev))
        return [{**{key: o[r0:r1] for key, o in zip(eng.WINDOW_KEYS, out)},
                 "window_starts": (widx0 + torch.arange(n, dtype=torch.int64)) * stride}
                for s, f0, f1, r0, r1, widx0, n in per_stream(self.frames_seen, self.windows_emitted, ks, T, stride)]
