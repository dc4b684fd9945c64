"""Drop-in for avenue_training_script_bbox.py's clip scorer (config 5) on the HIP plan (``vad_bbox_*``).

``CausalAnomalyDetector`` (bbox:51-101) keeps the class name, constructor, submodule names (state_dict keys
``encoder.0.weight`` ...) and forward return ``(anomaly_score.squeeze(), causal_adj (B,16,16), features (B,1024))``;
it runs in eval mode (the reference only ever scores clips with it: AnomalyVisualizer, bbox:339-368).
``AnomalyVisualizer.predict_anomaly_for_clip`` mirrors bbox:339-368; ``predict_clips`` scores a list of clips of
mixed lengths T by packing them into one batch per T (no layer couples clips, so this is exact).
``CausalAnomalyDetector.score_video`` scores the sliding windows of a planar RGB video (N, 3, H, W) without building
clips: the first layer reads window b's frames in place (``vad_bbox_windows_forward``);
``AnomalyVisualizer.extract_anomalous_frames`` is bbox:359-430 on it -- colour frames of any size go through one
table-form colour ingest per folder (``data.U8Ingest.table(..., color="rgb", planes=3)``).  The reference's person
detectors and drawing code (cv2 / yolov5) are out of scope.
"""
from __future__ import annotations

from collections import defaultdict
from pathlib import Path

import numpy as np
import torch
import torch.nn as nn

from . import _native as nat
from ._flat import FlatEngine, FlatPlan


class CausalAnomalyDetector(nn.Module):
    """bbox:51-101"""

    def __init__(self, input_channels=3, hidden_dim=64, num_frames=8):
        super().__init__()
        self.num_frames = num_frames
        self.encoder = nn.Sequential(
            nn.Conv3d(input_channels, 32, kernel_size=3, stride=1, padding=1), nn.ReLU(), nn.MaxPool3d(2),
            nn.Conv3d(32, 64, kernel_size=3, stride=1, padding=1), nn.ReLU(), nn.AdaptiveAvgPool3d((1, 4, 4)))
        self.feature_dim = 64 * 16
        self.causal_net = nn.Sequential(nn.Linear(self.feature_dim, 256), nn.ReLU(), nn.Linear(256, 16 * 16))
        self.classifier = nn.Sequential(nn.Linear(self.feature_dim, 128), nn.ReLU(), nn.Dropout(0.3),
                                        nn.Linear(128, 1), nn.Sigmoid())
        self._engine = None

    def forward(self, x):
        if self.training:
            raise NotImplementedError("the HIP bbox scorer runs in eval mode (call .eval(); the reference never "
                                      "trains this model)")
        if x.dim() != 5 or x.shape[1] != 3:
            raise ValueError(f"Expected (B,3,T,H,W) clips, got {tuple(x.shape)}")
        nat.require_hip(x)
        e = self._engine
        if e is None or e.device != x.device:
            e = self._engine = BboxEngine(self, x.device)
        s, adj, f = e.forward(x.float().contiguous())
        return s.squeeze(), adj, f

    def score_video(self, frames, window=None, stride=4, batch=64) -> dict:
        """Score every full window ``range(0, N - window + 1, stride)`` of a video: frames fp32 (N, 3, H, W) on the
        device, planar RGB in 0..1 (``data.ingest_u8(u8, (64, 64), 1, color=..., planes=3)`` builds them from camera
        bytes); window defaults to num_frames.  Windows run ``batch`` at a time, the ragged last batch on a plan of its
        own size, and are never copied into clips.  Returns anomaly_scores (W,), causal_graphs (W, 16, 16), features
        (W, 1024) -- for window w what ``model(clip)`` returns for frames[start:start + window] as a (3, T, H, W) clip
        -- and window_starts (W,) int64 on the host.  Eval mode only."""
        window = self.num_frames if window is None else window
        x = check_score_video(self, frames, window, stride, batch)
        window, stride, batch = int(window), int(stride), int(batch)
        nat.require_hip(x)
        e = self._engine
        if e is None or e.device != x.device:
            e = self._engine = BboxEngine(self, x.device)
        return e.score_video(x.float().contiguous(), window, stride, batch)

    def scoring_engine(self, device) -> "BboxEngine":
        e = self._engine
        if e is None or e.device != device:
            e = self._engine = BboxEngine(self, device)
        return e

    def open_stream(self, window=None, stride=1, *, max_push=1, frame_size=None):
        """A clip_stream.ClipStream on this model: push frames (k, 3, H, W) as they arrive, get score_video's keys for
        the windows they complete, read from a ring of window + max_push - 1 raw frames (``vad_bbox_ring_forward``)."""
        from .clip_stream import ClipStream
        window = self.num_frames if window is None else window
        return ClipStream(self, "bbox", window, stride, max_push=max_push, frame_size=frame_size)

    def open_stream_group(self, num_streams, window=None, stride=1, *, max_push=1, frame_size=None):
        """A clip_stream_group.ClipStreamGroup on this model: num_streams cameras of one frame size, one windows call
        per push for the windows of all of them (``vad_bbox_windows_forward_group``); window defaults to
        num_frames."""
        from .clip_stream_group import ClipStreamGroup
        window = self.num_frames if window is None else window
        return ClipStreamGroup(self, "bbox", num_streams, window, stride, max_push=max_push, frame_size=frame_size)


def check_score_video(model, frames, window, stride, batch) -> torch.Tensor:
    """The ValueErrors of score_video, raised before any device work; returns the frames."""
    if model.training:
        raise ValueError("score_video runs in eval mode (the HIP bbox scorer has no training path): call model.eval()")
    if not isinstance(frames, torch.Tensor) or frames.dim() != 4 or frames.shape[1] != 3:
        raise ValueError("score_video: frames of shape (N, 3, H, W), planar RGB, got "
                         f"{tuple(getattr(frames, 'shape', ())) or type(frames).__name__}")
    if not frames.is_floating_point():
        raise ValueError(f"score_video: frames must be floating point in 0..1 (uint8 frames go through "
                         f"data.ingest_u8(..., planes=3) first), got {frames.dtype}")
    if frames.shape[2] < 2 or frames.shape[3] < 2:
        raise ValueError(f"score_video: frames of at least 2 x 2 pixels (MaxPool3d(2)), got {tuple(frames.shape)}")
    for name, v, least in (("window", window, 2), ("stride", stride, 1), ("batch", batch, 1)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or int(v) != v or v < least:
            raise ValueError(f"score_video: {name} must be an integer >= {least}, got {v}")
    if frames.shape[0] < window:
        raise ValueError(f"score_video: the video has {frames.shape[0]} frames, fewer than one window of {window}")
    return frames


def clip_starts(n_frames: int, clip: int = 8, stride: int = 4) -> list:
    """The clips extract_anomalous_frames scores in a folder of n_frames frames, as the reference enumerates them
    (bbox:392): ``range(0, n_frames - clip, stride)`` -- not ``n_frames - clip + 1``, so a last clip that ends exactly
    on the last frame is left out (16 frames: starts 0 and 4)."""
    return list(range(0, n_frames - clip, stride))


class _BboxPlan(FlatPlan):
    @staticmethod
    def create_args(B, C, T, H, W):
        return B, T, H, W


class BboxEngine(FlatEngine):
    PLAN = _BboxPlan

    def __init__(self, model, device):
        super().__init__(model, device, "bbox", replace_params=True, opt_state=None, bind_names=("params",),
                         name_mismatch=(NotImplementedError,
                                        "the HIP bbox plan supports the reference layout (input_channels=3) only"))

    def forward(self, x):
        p = self.plan(*x.shape)
        B = x.shape[0]
        f = dict(dtype=torch.float32, device=self.device)
        s, adj, feats = torch.empty(B, **f), torch.empty(B, 16, 16, **f), torch.empty(B, 1024, **f)
        nat.check(nat.lib().vad_bbox_forward(p.h, nat.ptr(x), nat.ptr(s), nat.ptr(adj), nat.ptr(feats),
                                             nat.stream_of(self.device)))
        return s.view(B, 1), adj, feats

    WINDOW_KEYS = ("anomaly_scores", "causal_graphs", "features")

    def window_outputs(self, n):
        f = dict(dtype=torch.float32, device=self.device)
        return torch.empty(n, **f), torch.empty(n, 16, 16, **f), torch.empty(n, 1024, **f)

    def windows_forward(self, frames, first, stride, ring, nw, T, B, out):
        """nw windows of frames (n, 3, H, W) -- a video (ring 0) or a ring of `ring` slots -- into the tensors out
        (window_outputs' order), on the plan of exactly nw clips (B, the most a caller will ask for, is not used)."""
        n, _, H, W = frames.shape
        p = self.plan(nw, 3, T, H, W)
        nat.check(nat.lib().vad_bbox_ring_forward(p.h, nat.ptr(frames), n, first, stride, ring, *map(nat.ptr, out),
                                                  nat.stream_of(self.device)))

    def windows_forward_group(self, ring, cap, h_win, nw, dev_table, T, B, out):
        """nw windows of a group's rings (total_slots, 3, H, W), cap slots each, through the host rows h_win (nw, 2)
        int64 and the caller's device table (vad_bbox_windows_forward_group), into the tensors out; on the plan of
        exactly nw clips, as windows_forward."""
        n, _, H, W = ring.shape
        p = self.plan(nw, 3, T, H, W)
        nat.check(nat.lib().vad_bbox_windows_forward_group(p.h, nat.ptr(ring), n, cap, h_win.data_ptr(), nw,
                                                           nat.ptr(dev_table), *map(nat.ptr, out),
                                                           nat.stream_of(self.device)))

    def score_video(self, x, window, stride, batch) -> dict:
        """x (N, 3, H, W) fp32 contiguous on the engine's device, checked."""
        N, _, H, W = x.shape
        Wn = (N - window) // stride + 1
        f = dict(dtype=torch.float32, device=self.device)
        s, adj, feats = torch.empty(Wn, **f), torch.empty(Wn, 16, 16, **f), torch.empty(Wn, 1024, **f)
        fwd = nat.lib().vad_bbox_windows_forward
        for w0 in range(0, Wn, batch):
            p = self.plan(min(batch, Wn - w0), 3, window, H, W)
            nat.check(fwd(p.h, nat.ptr(x), N, w0 * stride, stride, nat.ptr(s[w0:]), nat.ptr(adj[w0:]),
                          nat.ptr(feats[w0:]), nat.stream_of(self.device)))
        return {"anomaly_scores": s, "causal_graphs": adj, "features": feats,
                "window_starts": torch.arange(Wn, dtype=torch.int64) * stride}


_EXTS_FRAMES = ("*.jpg", "*.jpeg", "*.png", "*.bmp")  # bbox:382


class AnomalyVisualizer:
    """The model-facing part of bbox:103-430: checkpoint loading, clip scoring and the scan of frame folders."""

    def __init__(self, model_path: str | None = None, device="cuda"):
        self.device = device
        self.model = self.load_trained_model(model_path)

    def load_trained_model(self, model_path):
        model = CausalAnomalyDetector().to(self.device)
        if model_path and Path(model_path).exists():
            ck = torch.load(model_path, map_location="cpu", weights_only=True)
            sd = ck.get("model_state_dict", ck.get("state_dict", ck)) if isinstance(ck, dict) else ck
            model.load_state_dict(sd)
        model.eval()
        return model

    def predict_anomaly_for_clip(self, video_clip):
        """bbox:339-368: one (3,T,H,W) clip (numpy or tensor) -> (score, causal graph (16,16), features (1024,))."""
        t = torch.from_numpy(video_clip).float() if isinstance(video_clip, np.ndarray) else video_clip.float()
        if t.dim() == 4:
            t = t.unsqueeze(0)
        with torch.no_grad():
            s, adj, f = self.model(t.to(self.device))
        return float(s.squeeze().cpu().numpy()), adj.squeeze().cpu().numpy(), f.squeeze().cpu().numpy()

    def predict_clips(self, clips, process_group=None):
        """Score clips of mixed lengths: one packed batch per T; results in input order.

        Data parallel (BASELINE config 5): with an initialised process group of world size P every rank passes the
        same clip list, scores the clips of each length group at positions r, r+P, ... (an even share of every T
        bucket), and the (score, graph, features) triples are exchanged with one all_gather_object at the end;
        no layer couples clips, so the result equals the single-process one."""
        import torch.distributed as dist
        world = dist.get_world_size(process_group) if dist.is_available() and dist.is_initialized() else 1
        rank = dist.get_rank(process_group) if world > 1 else 0
        groups = defaultdict(list)
        for i, c in enumerate(clips):
            t = torch.from_numpy(c).float() if isinstance(c, np.ndarray) else c.float()
            groups[tuple(t.shape)].append((i, t))
        mine = {}
        with torch.no_grad():
            for shape, items in groups.items():
                items = items[rank::world]
                if not items:
                    continue
                x = torch.stack([t for _, t in items]).to(self.device)
                s, adj, f = self.model(x)
                s = s.reshape(-1).cpu().numpy()
                adj, f = adj.cpu().numpy(), f.cpu().numpy()
                for k, (i, _) in enumerate(items):
                    mine[i] = (float(s[k]), adj[k], f[k])
        if world > 1:
            parts = [None] * world
            dist.all_gather_object(parts, mine, group=process_group)
            for p in parts:
                mine.update(p)
        return [mine[i] for i in range(len(clips))]

    def extract_anomalous_frames(self, video_dir, threshold: float = 0.3) -> list:
        """bbox:359-430 without its prints: every sub-folder of video_dir (sorted) with at least 8 frames (*.jpg,
        *.jpeg, *.png, *.bmp, sorted) is scored in clips of 8 frames at stride 4 (``clip_starts``: the reference's
        enumeration) and the clips with score > threshold come back as dicts video_id, start_frame, end_frame,
        frame_paths, anomaly_score, causal_graph (16, 16), features (1024,).

        Frames are decoded with PIL (``convert("RGB")``; the reference's cv2 decoder may differ on JPEG) at their own
        sizes; one table-form colour ingest per folder resizes them to 64 x 64 as data.resize_u8 does per channel and
        divides by 255 into planar RGB on the device (the reference's cv2.resize -> BGR2RGB -> / 255), and one
        score_video call scores the folder."""
        from PIL import Image

        from .data import U8Ingest
        video_dir = Path(video_dir)
        if not video_dir.exists():
            return []
        dev = next(self.model.parameters()).device
        ingest = None
        found = []
        for video_path in sorted(d for d in video_dir.iterdir() if d.is_dir()):
            frame_files = sorted(p for ext in _EXTS_FRAMES for p in video_path.glob(ext))
            starts = clip_starts(len(frame_files))
            if len(frame_files) < 8 or not starts:
                continue
            frames = []
            for path in frame_files:
                with Image.open(path) as im:
                    frames.append(torch.from_numpy(np.array(im.convert("RGB"), dtype=np.uint8))[None])
            if ingest is None:
                ingest = U8Ingest(dev)
            x = ingest.table(frames, len(frames), (64, 64), 1, color="rgb", planes=3)
            with torch.no_grad():
                o = self.model.score_video(x, window=8, stride=4)
            scores = o["anomaly_scores"].cpu().numpy()
            graphs, feats = o["causal_graphs"].cpu().numpy(), o["features"].cpu().numpy()
            for w, start in enumerate(starts):
                assert int(o["window_starts"][w]) == start
                score = float(scores[w])
                if score > threshold:
                    found.append({"video_id": video_path.name, "start_frame": start, "end_frame": start + 8,
                                  "frame_paths": frame_files[start:start + 8], "anomaly_score": score,
                                  "causal_graph": graphs[w], "features": feats[w]})
        return found
