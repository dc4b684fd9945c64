"""Sliding-window scoring of a whole video with CausalAnomalyDetector (eval mode, forward only).

The reference scores a video clip by clip (test_model, causal_anomaly_detection.py:1210-1232, over the clips its
test loader enumerates at stride T/2, cad:57), so every frame pays for the backbone once per clip that holds it.  In
eval mode BatchNorm normalises with its running statistics, so everything up to and including the per-frame part of
the causal head (backbone, pooled features, detector, box decode, ReID, GRU input projection) depends on the frame
alone.  score_video runs that part once per frame into a frame cache (vad_cad_frames_forward), then the per-window
part -- temporal mean, direct classifier, GRU recurrence, VAE / structure / dynamics / scorers, blend -- on windows
that read frames ``start + t`` of the cache (vad_cad_windows_forward).

Window w (frames ``w * stride .. w * stride + window - 1``) returns what ``model.eval(); model(clip, seed=seed,
step=step, clip0=clip0 + w)`` returns for that clip: the VAE noise the reference draws in eval mode too (cad:328-331)
is keyed by (seed, step, clip index), and window w takes the key of clip ``clip0 + w``.
"""
from __future__ import annotations

import torch

from . import _native as nat

MAX_DET, NUM_FACTORS = 5, 6
_CACHE_FIELDS = {"feats": 0, "gi": 1, "boxes": 2, "counts": 3, "slot": 4}


def check_arguments(model, frames, window, stride, chunk) -> torch.Tensor:
    """The ValueErrors of score_video, raised before any device work; returns the frames as (N, 1, H, W)."""
    if model.training:
        raise ValueError("score_video runs in eval mode (running BatchNorm statistics, no dropout): call model.eval()")
    if getattr(model, "_compute_dtype", torch.float32) != torch.float32:
        raise ValueError("score_video computes in fp32 only: set_compute_dtype(torch.float32) first")
    if not isinstance(frames, torch.Tensor) or frames.dim() not in (4, 5):
        raise ValueError("score_video: frames of shape (N, 1, H, W) or (1, N, 1, H, W), got "
                         f"{tuple(getattr(frames, 'shape', ()))}")
    if frames.dim() == 5:
        if frames.shape[0] != 1:
            raise ValueError(f"score_video: one video per call, got a batch of {frames.shape[0]}")
        frames = frames[0]
    if frames.shape[1] != 1:
        raise ValueError("ResNetBackbone here takes single-channel frames (input_channels=1, cad:515)")
    for name, v in (("window", window), ("stride", stride), ("chunk", chunk)):
        if int(v) != v or v < 1:
            raise ValueError(f"score_video: {name} must be an integer >= 1, got {v}")
    if frames.shape[0] < window:
        raise ValueError(f"score_video: the video has {frames.shape[0]} frames, fewer than one window of {window}")
    return frames


def cache_field(cache: torch.Tensor, n_frames: int, name: str) -> torch.Tensor:
    """View of one field of a frame cache: feats (N, 6144), gi (N, 5, 192), boxes (N, 5, 4) fp32; counts (N,),
    slot (N, 5) int32."""
    L = nat.lib()
    off = L.vad_cad_frame_cache_offset(n_frames, _CACHE_FIELDS[name])
    if off < 0:
        nat.check(1)
    shape = {"feats": (n_frames, 6144), "gi": (n_frames, MAX_DET, 192), "boxes": (n_frames, MAX_DET, 4),
             "counts": (n_frames,), "slot": (n_frames, MAX_DET)}[name]
    n = 1
    for s in shape:
        n *= s
    v = cache[off:off + n]
    if name in ("counts", "slot"):
        v = v.view(torch.int32)
    return v.view(shape)


def score_video(model, frames, window=16, stride=1, *, chunk=128, seed=0, step=0, clip0=0) -> dict:
    x = check_arguments(model, frames, window, stride, chunk)
    window, stride, chunk = int(window), int(stride), int(chunk)
    eng = model.engine()
    nat.require_hip(x)
    L = nat.lib()
    dev = eng.device
    x = x.contiguous().float()
    N, _, H, W = x.shape
    Wn = (N - window) // stride + 1
    stream = nat.stream_of(dev)
    # a forward armed for another input must not outlive this call (CadEngine.input_ready)
    armed, eng._armed = getattr(eng, "_armed", None), None
    if armed is not None:
        nat.check(L.vad_cad_set_option(armed.h, b"input_armed", 0))
    nfl = L.vad_cad_frame_cache_floats(N)
    if nfl < 0:
        nat.check(1)
    cache = torch.empty(nfl, dtype=torch.float32, device=dev)
    # per-frame stage, a chunk of F frames at a time on a (F, 1, H, W) plan: its per-clip buffers then have F rows,
    # which the windowed stage below uses for batches of F windows; the ragged last chunk takes a plan of its own size
    F = min(chunk, N)
    # (the plans' activations are overwritten: a backward still pending on an earlier forward must not read them)
    eng.generation += 1
    for f0 in range(0, N, F):
        n = min(F, N - f0)
        pl = eng.plan(n, 1, H, W)
        eng._set_stem_grad(pl)
        eng._check_images(pl)
        nat.check(L.vad_cad_frames_forward(pl.h, x[f0:f0 + n].data_ptr(), N, cache.data_ptr(), f0, stream))
    o = dict(final=torch.empty(Wn, device=dev), probs=torch.empty(Wn, 2, device=dev),
             causal=torch.empty(Wn, device=dev), kl=torch.empty(Wn, device=dev),
             z=torch.empty(Wn, MAX_DET, NUM_FACTORS, device=dev),
             adj=torch.empty(Wn, NUM_FACTORS, NUM_FACTORS, device=dev),
             nmax=torch.empty(Wn, dtype=torch.int32, device=dev))
    pl = eng.plan(F, 1, H, W)
    for w0 in range(0, Wn, F):
        nw = min(F, Wn - w0)
        nat.check(L.vad_cad_windows_forward(
            pl.h, cache.data_ptr(), N, window, stride, w0, nw, seed & ((1 << 64) - 1), step, clip0,
            o["final"][w0:].data_ptr(), o["probs"][w0:].data_ptr(), o["causal"][w0:].data_ptr(),
            o["kl"][w0:].data_ptr(), o["z"][w0:].data_ptr(), o["adj"][w0:].data_ptr(), o["nmax"][w0:].data_ptr(),
            stream))
    nm = o["nmax"].tolist()
    boxes = cache_field(cache, N, "boxes").clone()
    cnt = cache_field(cache, N, "counts").tolist()
    return {
        "anomaly_scores": o["final"],
        "direct_predictions": o["probs"],
        "causal_anomaly_scores": o["causal"],
        "kl_losses": o["kl"],
        "adjacency_matrices": o["adj"],
        "causal_factors": [o["z"][w, :nm[w]] for w in range(Wn)],
        "detections": [boxes[f, :cnt[f]] for f in range(N)],
        "window_starts": torch.arange(Wn, dtype=torch.int64) * stride,
    }
