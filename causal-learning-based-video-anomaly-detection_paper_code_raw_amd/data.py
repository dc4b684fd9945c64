"""Host data path of the training loop: frame folders -> u8 clips -> pinned staging -> HBM.

The reference decodes every frame with cv2/PIL into float tensors on the host (UCSDped2Dataset.__getitem__,
causal_anomaly_detection.py:85-104; UCSDped2SimpleDataset, minicausal_vad_complete3.py:192-216) and copies fp32
clips to the device inside the step (cad:639, mc:266).  Here the loader keeps clips as **u8** end to end:

* ``FrameFolderClips`` / ``FrameFolderClipsMC`` enumerate the same overlapping clips with the same (synthesised)
  labels as the reference datasets (cad:39-80, mc:104-190) and return ``(T, 1, H, W)`` / ``(1, T, H, W)`` uint8
  frames; decoding is PIL, resizing the native ``vad_resize_u8`` (cv2 INTER_LINEAR scheme, cad:88-89).
* ``ClipStager`` keeps u8 batches in pinned host memory, copies them to the device as u8 and converts them to fp32
  there (``vad_u8_to_clip``: the reference's Normalize(0.5, 0.5) over raw 0..255 pixels, or ToTensor's /255), both
  on a stream of its own -- a quarter of the PCIe bytes of fp32 clips, and batch k+1's staging overlaps step k.
* ``prefetch(loader, stager)`` yields device clips one batch ahead.
"""
from __future__ import annotations

import ctypes
import os
import random

import numpy as np
import torch

from . import _native as nat

_EXTS_CAD = (".jpg", ".png", ".tif")


def _decode_gray(path: str, size_hw: tuple[int, int] | None, pil_resize: bool = False) -> np.ndarray:
    """One frame as (H, W) uint8 grayscale (PIL's ITU-R 601 luma for colour frames), resized to size_hw when given:
    cad: cv2.imread GRAYSCALE + cv2.resize (cad:87-88) -> the native bilinear; mc: PIL + torchvision Resize, which
    is PIL's own bilinear resize (mc:117-119) -> pil_resize=True."""
    from PIL import Image
    with Image.open(path) as im:
        g = im.convert("L")
        if pil_resize and size_hw is not None and g.size != (size_hw[1], size_hw[0]):
            g = g.resize((size_hw[1], size_hw[0]), Image.BILINEAR)
        a = np.asarray(g, dtype=np.uint8)
    if size_hw is not None and a.shape != tuple(size_hw):
        return resize_u8(a, *size_hw)
    return np.ascontiguousarray(a)


COLOR_FORMATS = ("rgb", "bgr", "rgbx", "bgrx")  # packed pixel layouts; the index is the library's fmt


def _color_format(color, what):
    """(fmt, bytes per pixel) of a packed colour format name (ValueError for anything else)."""
    if not isinstance(color, str) or color not in COLOR_FORMATS:
        raise ValueError(f"{what}: color must be None or one of {COLOR_FORMATS}, got {color!r}")
    fmt = COLOR_FORMATS.index(color)
    return fmt, 4 if fmt >= 2 else 3


def luma_u8(frames, color: str) -> np.ndarray:
    """Grey of packed colour frames, uint8 (k, Hs, Ws, C) or (Hs, Ws, C) with C = 3 (rgb, bgr) or 4 (rgbx, bgrx; the
    fourth byte is not read) -> (k, Hs, Ws) or (Hs, Ws): L = (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16, PIL's
    convert("L") (native vad_luma_u8).  ``ingest_u8(frames, size, mode, color=color)`` equals luma_u8 -> resize_u8 ->
    the mode's float32 expression."""
    fmt, step = _color_format(color, "luma_u8")
    a = frames.numpy() if isinstance(frames, torch.Tensor) else np.asarray(frames)
    if a.dtype != np.uint8 or a.ndim not in (3, 4) or a.shape[-1] != step or a.shape[-2] < 1 or a.shape[-3] < 1:
        raise ValueError(f"luma_u8: uint8 frames (k, Hs, Ws, {step}) or (Hs, Ws, {step}) for color={color!r}, got "
                         f"{a.dtype} {tuple(a.shape)}")
    hs, ws = a.shape[-3:-1]
    if a.strides[-1] != 1 or a.strides[-2] != step or (hs > 1 and a.strides[-3] < step * ws):
        a = np.ascontiguousarray(a)  # (rows may be strided; pixels and channels must be packed)
    pitch = a.strides[-3] if hs > 1 else step * ws
    out = np.empty(a.shape[:-1], dtype=np.uint8)
    L = nat.lib()
    for src, dst in zip(a if a.ndim == 4 else [a], out if a.ndim == 4 else [out]):
        nat.check(L.vad_luma_u8(src.ctypes.data, hs, ws, pitch, fmt, dst.ctypes.data))
    return out


def resize_u8(img: np.ndarray, h: int, w: int) -> np.ndarray:
    """Bilinear resize of a (H, W) uint8 image (native vad_resize_u8)."""
    src = np.ascontiguousarray(img, dtype=np.uint8)
    dst = np.empty((h, w), dtype=np.uint8)
    nat.check(nat.lib().vad_resize_u8(src.ctypes.data, src.shape[0], src.shape[1], dst.ctypes.data, h, w))
    return dst


class FrameFolderClips(torch.utils.data.Dataset):
    """UCSDped2Dataset (cad:39-104): clips of ``sequence_length`` frames with stride sequence_length // 2 over every
    frame folder of ``root/split``; Train labels 0, Test labels from the reference's heuristic (cad:62-80, the same
    ``random.seed(folder_num * 1000 + i)`` draw).  Items: ((T, 1, 240, 360) uint8, int64 label)."""

    def __init__(self, root_dir, split="Train", sequence_length=16, frame_size=(240, 360)):
        self.root_dir = os.path.join(root_dir, split)
        self.sequence_length = sequence_length
        self.frame_size = frame_size
        self.sequences, self.labels = [], []
        T = sequence_length
        for folder in sorted(os.listdir(self.root_dir)):
            folder_path = os.path.join(self.root_dir, folder)
            if not os.path.isdir(folder_path):
                continue
            frames = sorted(f for f in os.listdir(folder_path) if f.endswith(_EXTS_CAD))
            for i in range(0, len(frames) - T + 1, T // 2):
                seq = frames[i:i + T]
                if len(seq) != T:
                    continue
                self.sequences.append((folder_path, seq, i))
                if split == "Train":
                    self.labels.append(0)
                    continue
                folder_num = int(folder.replace("Test", "").replace("Train", ""))
                progress = i / max(len(frames) - T, 1)
                p = 0.0
                if folder_num in (1, 3, 5, 7, 9, 11):
                    p += 0.4
                if progress > 0.6:
                    p += 0.3
                if 0.3 < progress < 0.7:
                    p += 0.2
                rnd = random.Random(folder_num * 1000 + i)  # == random.seed(...); random.random() (cad:78-79)
                self.labels.append(1 if rnd.random() < p else 0)

    def __len__(self):
        return len(self.sequences)

    def __getitem__(self, idx):
        folder_path, names, _ = self.sequences[idx]
        frames = np.stack([_decode_gray(os.path.join(folder_path, n), self.frame_size) for n in names])
        return torch.from_numpy(frames).unsqueeze(1), torch.tensor(self.labels[idx], dtype=torch.long)


class FrameFolderClipsMC(torch.utils.data.Dataset):
    """UCSDped2SimpleDataset (mc:104-216): .tif folders (``*_gt`` skipped), clips of ``temporal_frames`` at
    ``stride``, at most ``max_clips_per_video`` per video, the reference's label rule (mc:165-172).  Items:
    ((1, T, S, S) uint8, float32 label); the device conversion is ToTensor's /255 (mode 1)."""

    def __init__(self, root_dir, subset="Train", temporal_frames=8, spatial_size=64, max_clips_per_video=10,
                 stride=4):
        self.spatial_size = spatial_size
        self.video_clips, self.labels = [], []
        subset_path = os.path.join(root_dir, subset)
        if not os.path.exists(subset_path):
            raise ValueError(f"Path {subset_path} does not exist")
        folders = sorted(f for f in os.listdir(subset_path)
                         if os.path.isdir(os.path.join(subset_path, f)) and not f.endswith("_gt"))
        for video_idx, folder in enumerate(folders):
            vp = os.path.join(subset_path, folder)
            files = sorted(f for f in os.listdir(vp) if f.endswith(".tif"))
            if len(files) < temporal_frames:
                continue
            added = 0
            for start in range(0, len(files) - temporal_frames + 1, stride):
                if added >= max_clips_per_video:
                    break
                self.video_clips.append([os.path.join(vp, f) for f in files[start:start + temporal_frames]])
                label = (1 if (video_idx * added) % 5 == 0 else 0) if subset == "Train" else (1 if added % 2 == 0
                                                                                               else 0)
                self.labels.append(label)
                added += 1
        if len(set(self.labels)) < 2:
            # the reference's forced anomalies (mc:176-183): the same draw from numpy's global generator
            normal = [i for i, l in enumerate(self.labels) if l == 0]
            if normal:
                for i in np.random.choice(normal, min(len(normal) // 3, 10), replace=False):
                    self.labels[i] = 1

    def __len__(self):
        return len(self.video_clips)

    def __getitem__(self, idx):
        S = self.spatial_size
        frames = np.stack([_decode_gray(p, (S, S), pil_resize=True) for p in self.video_clips[idx]])
        return torch.from_numpy(frames).unsqueeze(0), torch.tensor(float(self.labels[idx]), dtype=torch.float32)


class _Staged:
    """An issued batch: its fp32 device clip (being written on the stager's stream) and the event that completes it."""
    __slots__ = ("out", "ready", "slot")

    def __init__(self, out, ready, slot):
        self.out, self.ready, self.slot = out, ready, slot


class ClipStager:
    """Pinned u8 staging + on-device u8 -> fp32 conversion on a stream of its own, one batch ahead of the step.

    ``issue(batch_u8)`` enqueues batch k+1's conversion while step k computes and returns a handle; ``finish(handle)``
    returns its fp32 device clip, ordered on the current stream (``wait=True``) or left to the consumer
    (``wait=False``: hand ``handle.ready`` to ``CadTrainer.step(inputs_ready=...)``, whose early stem waits for it on
    the plan's stem stream and the step's critical stream never does).  ``stage(batch)`` = ``finish(issue(batch))``.
    mode 0: (u8 - 0.5) / 0.5 (cad), 1: u8 / 255 (mc/bbox).

    direct=False (default): an H2D copy of the u8 batch into a device buffer (the copy engine), then the conversion,
    both on the stager's stream.  Nothing queued there waits for the step's streams: the u8 and fp32 device buffers
    are stream-ordered by the caching allocator (the fp32 clip recorded on its consumer's stream), which matters --
    HIP spreads streams over GPU_MAX_HW_QUEUES (4) hardware queues, and the previous design (a fixed device slot whose
    copy waited for an event of the step's stream) stalled whichever step stream shared the copy's queue: config 2 at
    3.0 ms/step on two of the four queues, 1.80 on the others; this one 1.75-1.83 ms on all four against 1.74 ms with
    clips already in HBM (profiles/r04_h2d_queues.json).  direct=True: the conversion kernel reads the pinned host
    batch itself over PCIe (``vad_host_device_ptr``), no copy engine and no u8 device buffer (1.86-1.93 ms: the
    PCIe-bound kernel holds CUs beside the step).

    A batch that is not pinned and contiguous goes through a ring of ``depth`` pinned buffers (a slot is refilled
    once its previous conversion has finished); a pinned batch is read in place and must not be overwritten until
    ``handle.ready`` has completed.  Each returned clip is a fresh tensor (recorded on the consuming stream)."""

    def __init__(self, device, mode=0, depth=2, direct=False):
        self.device = torch.device(device)
        nat.require_hip(torch.empty(0, device=self.device))
        self.mode = mode
        self.depth = depth
        self.direct = direct
        self.stream = torch.cuda.Stream(self.device)
        self.copy_stream = self.stream  # (the name of earlier releases)
        self._ring = []  # [pinned u8, device u8 (direct=False), conversion-done event]
        self._k = 0
        self._dptr = {}  # pinned host pointer -> its device address
        # direct mode: caller-owned pinned batches read in place over PCIe, kept alive until their conversion is done
        # (the caching host allocator records no event for a kernel's reads, so a dropped batch could be reused, e.g.
        # by a DataLoader pin thread, while the conversion still reads it)
        self._inflight = []

    def _slot(self, shape):
        if len(self._ring) <= self._k or tuple(self._ring[self._k][0].shape) != tuple(shape):
            slot = [torch.empty(shape, dtype=torch.uint8, pin_memory=True), None, torch.cuda.Event()]
            if len(self._ring) <= self._k:
                self._ring.append(slot)
            else:
                # (a shape change, e.g. the last partial batch: the old pinned buffer may still be read by its
                # conversion -- direct mode reads it over PCIe, with no host-allocator event -- before it is freed)
                self._ring[self._k][2].synchronize()
                self._ring[self._k] = slot
        return self._ring[self._k]

    def _device_address(self, host: torch.Tensor) -> int:
        p = host.data_ptr()
        d = self._dptr.get(p)
        if d is None:
            out = ctypes.c_void_p()
            nat.check(nat.lib().vad_host_device_ptr(p, ctypes.addressof(out)))
            d = self._dptr[p] = out.value
            if len(self._dptr) > 64:  # (caller-owned pinned batches come and go)
                self._dptr.pop(next(iter(self._dptr)))
        return d

    def issue(self, batch_u8: torch.Tensor) -> _Staged:
        """Enqueue one u8 batch's conversion (and, direct=False, its H2D copy) on the stager's stream."""
        if batch_u8.dtype != torch.uint8:
            raise TypeError("ClipStager.issue expects a uint8 batch")
        if batch_u8.numel() == 0:
            ev = torch.cuda.Event()
            ev.record(self.stream)
            return _Staged(torch.empty(batch_u8.shape, dtype=torch.float32, device=self.device), ev, None)
        if batch_u8.is_pinned() and batch_u8.is_contiguous() and batch_u8.data_ptr() % 16 == 0:
            src, slot, done = batch_u8, None, torch.cuda.Event()
        else:
            slot = self._slot(batch_u8.shape)
            self._k = (self._k + 1) % self.depth
            src, done = slot[0], slot[2]
            done.synchronize()  # the slot's previous conversion (or copy) has read the pinned buffer
            src.copy_(batch_u8)
        with torch.cuda.stream(self.stream):
            out = torch.empty(batch_u8.shape, dtype=torch.float32, device=self.device)
            if self.direct:
                sp = self._device_address(src)
            else:
                dev = torch.empty(batch_u8.shape, dtype=torch.uint8, device=self.device)
                dev.copy_(src, non_blocking=True)
                sp = dev.data_ptr()
            nat.check(nat.lib().vad_u8_to_clip(sp, src.numel(), self.mode, out.data_ptr(),
                                               ctypes.c_void_p(self.stream.cuda_stream)))
            done.record(self.stream)
        if self.direct and slot is None:
            self._inflight = [(b, e) for b, e in self._inflight if not e.query()]
            self._inflight.append((src, done))
        return _Staged(out, done, slot)

    def finish(self, handle: _Staged, wait: bool = True) -> torch.Tensor:
        """The fp32 device clip of an issued batch.  wait=True: ready on the current stream; wait=False: the consumer
        orders itself after ``handle.ready`` (e.g. CadTrainer.step(x, y, inputs_ready=handle.ready))."""
        cur = torch.cuda.current_stream(self.device)
        if wait:
            cur.wait_event(handle.ready)
        handle.out.record_stream(cur)  # (its memory is not reused before the current stream's queued work is done)
        return handle.out

    def stage(self, batch_u8: torch.Tensor) -> torch.Tensor:
        return self.finish(self.issue(batch_u8))


def prefetch(loader, stager: ClipStager, with_ready: bool = False):
    """Iterate (device clips, device labels) one batch ahead: the H2D copy of batch k+1 is issued before batch k is
    yielded (it runs on the copy stream while step k computes) and converted when batch k+1 is yielded.  uint8
    batches go through the stager; float batches (the reference's own datasets) are copied as they are.
    with_ready=True: yields (clips, labels, ready) -- for a staged batch the current stream does not wait for it and
    ``ready`` is the event that completes it (hand it to CadTrainer.step(inputs_ready=...)); None otherwise."""
    def issue(x, y):
        h = stager.issue(x) if x.dtype == torch.uint8 else x
        return h, y

    def finish(h, y):
        yd = y.to(stager.device, non_blocking=True)
        if isinstance(h, torch.Tensor):
            xd = h.to(stager.device, non_blocking=True)
            return (xd, yd, None) if with_ready else (xd, yd)
        if with_ready:
            return stager.finish(h, wait=False), yd, h.ready
        return stager.finish(h), yd

    it = iter(loader)
    try:
        pending = issue(*next(it))
    except StopIteration:
        return
    for x, y in it:
        cur = finish(*pending)
        pending = issue(x, y)
        yield cur
    yield finish(*pending)


# ---------------------------------------------------------------- scoring-side ingest
INGEST_MODES = (0, 1, 2)  # (u8 - 0.5) / 0.5 (cad), u8 / 255 (mc, bbox), clamp(u8 / 255, 0.001, 0.999) (cad1:110-114)


def check_u8_frames(frames, what="ingest_u8", color=None) -> torch.Tensor:
    """The ValueErrors of a u8 source, raised before any device work: a uint8 tensor (k, Hs, Ws) or (k, 1, Hs, Ws)
    with Hs, Ws >= 1.  Returns it as (k, Hs, Ws) (a view).  With a colour format: a uint8 tensor (k, Hs, Ws, C) of
    packed pixels, C = 3 (rgb, bgr) or 4 (rgbx, bgrx), returned as it is."""
    if color is not None:
        _, step = _color_format(color, what)
        if not isinstance(frames, torch.Tensor) or frames.dim() != 4:
            raise ValueError(f"{what}: color={color!r} takes uint8 frames of shape (k, Hs, Ws, {step}), got "
                             f"{tuple(getattr(frames, 'shape', ())) or type(frames).__name__}")
        if frames.dtype != torch.uint8:
            raise ValueError(f"{what}: frames must be uint8, got {frames.dtype}")
        if frames.shape[3] != step:
            raise ValueError(f"{what}: color={color!r} has {step} bytes per pixel, but the last dimension of the "
                             f"frames {tuple(frames.shape)} is {frames.shape[3]}")
        if frames.shape[1] < 1 or frames.shape[2] < 1:
            raise ValueError(f"{what}: empty frames {tuple(frames.shape)}")
        return frames
    if not isinstance(frames, torch.Tensor) or frames.dim() not in (3, 4):
        raise ValueError(f"{what}: uint8 frames of shape (k, Hs, Ws) or (k, 1, Hs, Ws), got "
                         f"{tuple(getattr(frames, 'shape', ())) or type(frames).__name__}")
    if frames.dtype != torch.uint8:
        raise ValueError(f"{what}: frames must be uint8, got {frames.dtype}")
    if frames.dim() == 4:
        if frames.shape[1] != 1:
            raise ValueError(f"{what}: single-channel frames only, got {frames.shape[1]} channels")
        frames = frames[:, 0]
    if frames.shape[1] < 1 or frames.shape[2] < 1:
        raise ValueError(f"{what}: empty frames {tuple(frames.shape)}")
    return frames


def _check_size_mode(size_hw, mode, what="ingest_u8"):
    try:
        h, w = (int(v) for v in size_hw)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: size_hw must be (H, W), got {size_hw!r}") from None
    if h < 1 or w < 1 or (h, w) != tuple(size_hw):
        raise ValueError(f"{what}: size_hw must be two integers >= 1, got {size_hw!r}")
    if mode not in INGEST_MODES:
        raise ValueError(f"{what}: mode 0 ((u8 - 0.5) / 0.5), 1 (u8 / 255) or 2 (u8 / 255 clamped to 0.001..0.999), "
                         f"got {mode!r}")
    return h, w


def _check_planes(planes, color, what="ingest_u8") -> int:
    if isinstance(planes, bool) or planes not in (1, 3):
        raise ValueError(f"{what}: planes must be 1 (grey) or 3 (planar RGB), got {planes!r}")
    if planes == 3 and color is None:
        raise ValueError(f"{what}: planes=3 needs colour frames (color= one of {COLOR_FORMATS})")
    return int(planes)


def ingest_device(model, sources, what) -> torch.device:
    """The device a push_u8 runs on: the model's, which must be a HIP device -- it reads host sources -- and the one
    every device source is on (ValueError, before any device work)."""
    dev = next(model.parameters()).device
    for x in sources:
        if dev.type != "cuda" or (x.is_cuda and x.device != dev):
            raise ValueError(f"{what}: frames on {x.device}, but the model is on {dev} (host frames are read by the "
                             "model's HIP device; device frames must be on it)")
    return dev


class U8Ingest:
    """u8 frames at the source's own size -> fp32 (k, 1, H, W) on the device, resized as ``resize_u8`` resizes and
    normalised, in one launch on the current stream (vad_ingest_u8 / vad_ingest_u8_table; packed colour frames
    (k, Hs, Ws, C) with ``color``: vad_ingest_u8_color / _table, grey by ``luma_u8`` or, with planes=3, the planes
    R, G, B as (k, 3, H, W)).  Holds what that needs
    besides the kernel: a pinned slot for pageable sources, the device addresses of pinned sources it has seen, and --
    once ``table`` is used -- the pinned frame table with its device copy.

    A source may be on the device, in pinned host memory (read in place over PCIe: it must stay unchanged until the
    work queued by the call has run) or in pageable host memory (copied through the slot, which waits for the launch
    that last read it).  Rows may be strided; a source whose pixels within a row are not adjacent (colour: whose
    pixels are not ``step`` bytes apart with the channels packed) is made contiguous first."""

    def __init__(self, device):
        self.device = torch.device(device)
        self._slot = None   # pinned u8 bytes for pageable sources
        self._done = None   # the event behind the last launch: it has read the slot and the device has the table
        self._dptr = {}     # pinned host pointer -> its device address
        self._h_table = self._d_table = None

    def _address(self, host: torch.Tensor) -> int:
        p = host.data_ptr()
        d = self._dptr.get(p)
        if d is None:
            d = self._dptr[p] = nat.host_device_ptr(host)
            if len(self._dptr) > 256:  # (caller-owned pinned frames come and go)
                self._dptr.pop(next(iter(self._dptr)))
        return d

    def _wait(self):
        if self._done is not None:
            self._done.synchronize()

    def _record(self):
        if self._done is None:
            self._done = torch.cuda.Event()
        self._done.record(torch.cuda.current_stream(self.device))

    def _sources(self, chunks, step=1):
        """Per chunk (k, Hs, Ws), with step > 1 (k, Hs, Ws, step): (address of frame 0, Hs, Ws, row pitch, frame
        stride), strides in bytes."""
        def readable(x):  # rows of adjacent pixels, pitch >= Ws apart (not an expanded or transposed view)
            if step > 1 and x.stride(3) != 1:
                return False
            return (x.shape[2] == 1 or x.stride(2) == step) and (x.shape[1] == 1 or x.stride(1) >= step * x.shape[2])

        chunks = [x if readable(x) else x.contiguous() for x in chunks]
        pageable = [i for i, x in enumerate(chunks) if not x.is_cuda and not x.is_pinned()]
        if pageable:
            need = sum(chunks[i].numel() for i in pageable)
            self._wait()
            if self._slot is None or self._slot.numel() < need:
                self._slot = torch.empty(need, dtype=torch.uint8, pin_memory=True)
            off = 0
            for i in pageable:
                x = chunks[i]
                view = self._slot[off:off + x.numel()].view(x.shape)
                view.copy_(x)
                chunks[i] = view
                off += x.numel()
        out = []
        for x in chunks:
            if x.is_cuda:
                if x.device != self.device:
                    raise ValueError(f"ingest_u8: frames on {x.device}, the ingest runs on {self.device}")
                addr = x.data_ptr()
            else:
                addr = self._address(x)
            k, hs, ws = x.shape[:3]
            pitch = x.stride(1) if hs > 1 else step * ws
            fstride = x.stride(0) if k > 1 else 0
            out.append((addr, hs, ws, pitch, fstride))
        return out

    def _out(self, out, n, h, w, planes=1):
        if out is None:
            return torch.empty(n, planes, h, w, dtype=torch.float32, device=self.device)
        if (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != (n, planes, h, w)
                or not out.is_contiguous() or out.device != self.device or out.data_ptr() % 16):
            raise ValueError(f"ingest_u8: out must be a contiguous, 16-byte aligned float32 tensor ({n}, {planes}, {h}, "
                             f"{w}) on {self.device}")
        return out

    def ingest(self, frames, size_hw, mode, out=None, color=None, planes=1) -> torch.Tensor:
        """frames: uint8 (k, Hs, Ws) or (k, 1, Hs, Ws), k >= 1 -> fp32 (k, 1, H, W), the uniform form.  With
        color (one of COLOR_FORMATS): packed pixels (k, Hs, Ws, C) -> (k, planes, H, W)."""
        x = check_u8_frames(frames, color=color)
        planes = _check_planes(planes, color)
        h, w = _check_size_mode(size_hw, mode)
        if x.shape[0] < 1:
            raise ValueError("ingest_u8: no frame")
        nat.require_hip(torch.empty(0, device=self.device))
        out = self._out(out, x.shape[0], h, w, planes)
        fmt, step = (0, 1) if color is None else _color_format(color, "ingest_u8")
        (addr, hs, ws, pitch, fstride), = self._sources([x], step)
        with torch.cuda.device(self.device):
            if color is None:
                nat.check(nat.lib().vad_ingest_u8(addr, x.shape[0], hs, ws, pitch, fstride, h, w, mode, out.data_ptr(),
                                                  nat.stream_of(self.device)))
            else:
                nat.check(nat.lib().vad_ingest_u8_color(addr, x.shape[0], hs, ws, pitch, fstride, fmt, planes, h, w,
                                                        mode, out.data_ptr(), nat.stream_of(self.device)))
        self._record()
        return out

    def table(self, chunks, n, size_hw, mode, out=None, capacity=None, color=None, planes=1) -> torch.Tensor:
        """chunks: uint8 tensors (k_i, Hs_i, Ws_i), each of its own size -> fp32 (n, 1, H, W): their frames in order,
        then n - sum(k_i) frames of zeros, in one table-form launch.  capacity: the largest n this object will see
        (the tables are allocated once).  With color: chunks (k_i, Hs_i, Ws_i, C), all of that one format ->
        (n, planes, H, W)."""
        h, w = _check_size_mode(size_hw, mode)
        planes = _check_planes(planes, color)
        chunks = [check_u8_frames(x, color=color) for x in chunks]
        total = sum(x.shape[0] for x in chunks)
        if total < 1 or total > n:
            raise ValueError(f"ingest_u8: {total} frames for a batch of {n}")
        nat.require_hip(torch.empty(0, device=self.device))
        L = nat.lib()
        out = self._out(out, n, h, w, planes)
        fmt, step = (0, 1) if color is None else _color_format(color, "ingest_u8")
        cap = max(n, capacity or 0)
        if self._h_table is None or self._h_table.shape[0] < cap:
            nb = L.vad_ingest_table_bytes(cap)
            if nb < 0:
                nat.check(1)
            self._wait()
            self._h_table = torch.zeros(cap, 4, dtype=torch.int64).pin_memory()
            self._d_table = torch.zeros(nb // 8, dtype=torch.int64, device=self.device)
        srcs = self._sources(chunks, step)
        rows = [(addr + j * fstride, hs, ws, pitch) for x, (addr, hs, ws, pitch, fstride) in zip(chunks, srcs)
                for j in range(x.shape[0])]
        rows += [(0, 0, 0, 0)] * (n - total)
        self._wait()  # (the device has the table of the launch before)
        self._h_table[:n] = torch.tensor(rows, dtype=torch.int64)
        with torch.cuda.device(self.device):
            if color is None:
                nat.check(L.vad_ingest_u8_table(self._h_table.data_ptr(), n, h, w, mode, out.data_ptr(),
                                                self._d_table.data_ptr(), nat.stream_of(self.device)))
            else:
                nat.check(L.vad_ingest_u8_color_table(self._h_table.data_ptr(), n, fmt, planes, h, w, mode,
                                                      out.data_ptr(), self._d_table.data_ptr(),
                                                      nat.stream_of(self.device)))
        self._record()
        return out


_INGESTS = {}


def ingest_u8(frames, size_hw, mode, *, out=None, color=None, planes=1) -> torch.Tensor:
    """uint8 frames (k, Hs, Ws) or (k, 1, Hs, Ws) -> fp32 (k, 1, H, W) on the device, each frame resized to
    size_hw = (H, W) exactly as ``resize_u8`` resizes it and normalised (mode 0: (u8 - 0.5) / 0.5, 1: u8 / 255,
    2: u8 / 255 clamped to 0.001..0.999), by one kernel on the current stream.  frames on the HIP device, in pinned
    host memory (read in place) or in pageable host memory (through a pinned slot); host frames go to ``out``'s
    device, else the current one.  ``score_video(ingest_u8(video_u8, (H, W), 0))`` scores a u8 video.  The state
    lives in one U8Ingest per device; a stream owns its own.

    color ("rgb", "bgr", "rgbx" or "bgrx"): frames are packed colour pixels, uint8 (k, Hs, Ws, 3) or (k, Hs, Ws, 4)
    (the X byte is never read).  planes=1 -> (k, 1, H, W): ``luma_u8`` of the source, then the above.  planes=3 ->
    (k, 3, H, W): the planes R, G, B, each ``resize_u8`` of its channel and normalised --
    ``bbox_model.score_video(ingest_u8(video_u8, (64, 64), 1, color="bgr", planes=3))``."""
    x = check_u8_frames(frames, color=color)
    _check_planes(planes, color)
    if x.is_cuda:
        dev = x.device
    elif out is not None:
        dev = out.device
    else:
        nat.require_hip(torch.empty(0, device="cuda"))
        dev = torch.device("cuda", torch.cuda.current_device())
    ing = _INGESTS.get(dev)
    if ing is None:
        ing = _INGESTS[dev] = U8Ingest(dev)
    return ing.ingest(x, size_hw, mode, out=out, color=color, planes=planes)
