"""Sliding-window scoring of a whole video with the memory autoencoder (VideoAutoEncoder, eval mode, forward only).

The reference scores a video clip by clip (calculate_anomaly_scores, causal_anomaly_detection1.py:542-552, over the
clips its test set enumerates at stride T // 4, cad1:72), so every frame is encoded once per clip that holds it: four
times there, T times for a dense per-frame curve at stride 1.  In eval mode BatchNorm normalises with its running
statistics, so the four encoder convs, Linear(2048, 64) + tanh and the LSTM input projection W_ih x + b_ih depend on
the frame alone.  score_video runs that part once per frame into a frame cache (vad_ae_frames_forward), then the
per-window part -- the 64-wide LSTM recurrence over the window's cached rows, the memory-ring score, one decoder call
and the MSE of that one frame against the window's T frames -- on windows that read frames ``start + t``
(vad_ae_windows_forward).

Window w (frames ``w * stride .. w * stride + window - 1``) returns what ``model.eval()`` followed by the clip path
returns for that clip (AeTrainer.eval_batch, calculate_anomaly_scores).
"""
from __future__ import annotations

import torch

from . import _native as nat

LATENT, HW = 64, 64
_CACHE_FIELDS = {"lat": (0, LATENT), "gx": (1, 4 * LATENT)}


def check_arguments(model, frames, window, stride, chunk) -> torch.Tensor:
    """The ValueErrors of score_video, raised before any device work; returns the frames as (N, 1, 64, 64)."""
    if model.training:
        raise ValueError("score_video runs in eval mode (running BatchNorm statistics): call model.eval()")
    if not isinstance(frames, torch.Tensor) or frames.dim() not in (4, 5):
        raise ValueError("score_video: frames of shape (N, 1, 64, 64) or (1, N, 1, 64, 64), got "
                         f"{tuple(getattr(frames, 'shape', ()))}")
    if frames.dim() == 5:
        if frames.shape[0] != 1:
            raise ValueError(f"score_video: one video per call, got a batch of {frames.shape[0]}")
        frames = frames[0]
    if tuple(frames.shape[1:]) != (1, HW, HW):
        raise ValueError("score_video: frames of shape (N, 1, 64, 64) (the encoder's Linear(128*4*4) fixes 64x64 "
                         f"single-channel frames, cad1:151), got {tuple(frames.shape)}")
    for name, v in (("window", window), ("stride", stride), ("chunk", chunk)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or int(v) != v or v < 1:
            raise ValueError(f"score_video: {name} must be an integer >= 1, got {v}")
    if frames.shape[0] < window:
        raise ValueError(f"score_video: the video has {frames.shape[0]} frames, fewer than one window of {window}")
    return frames


def cache_field(cache: torch.Tensor, n_frames: int, name: str) -> torch.Tensor:
    """View of one field of a frame cache: lat (N, 64), gx (N, 256)."""
    field, width = _CACHE_FIELDS[name]
    off = nat.lib().vad_ae_frame_cache_offset(n_frames, field)
    if off < 0:
        nat.check(1)
    return cache[off:off + n_frames * width].view(n_frames, width)


def score_video(model, frames, window=16, stride=1, *, chunk=256, return_reconstructions=False) -> dict:
    x = check_arguments(model, frames, window, stride, chunk)
    window, stride, chunk = int(window), int(stride), int(chunk)
    nat.require_hip(x)
    eng = model.engine()
    L = nat.lib()
    dev = eng.device
    x = x.to(torch.float32).contiguous()
    N = int(x.shape[0])
    Wn = (N - window) // stride + 1
    stream = eng.stream()
    nfl = L.vad_ae_frame_cache_floats(N)
    if nfl < 0:
        nat.check(1)
    cache = torch.empty(nfl, dtype=torch.float32, device=dev)
    # per-frame stage, a chunk of F frames at a time on a (F, 1) plan: its per-clip buffers then have F rows, which the
    # windowed stage below uses for batches of F windows; the ragged last chunk takes a plan of its own size.  (The
    # ring holds 500 rows and a plan at most as many clips.)
    F = min(chunk, N, 500)
    for f0 in range(0, N, F):
        n = min(F, N - f0)
        nat.check(L.vad_ae_frames_forward(eng.plan(n, 1).h, x[f0:f0 + n].data_ptr(), N, cache.data_ptr(), f0, stream))
    o = dict(seq=torch.empty(Wn, LATENT, device=dev), err=torch.empty(Wn, device=dev),
             mem=torch.empty(Wn, device=dev), score=torch.empty(Wn, device=dev))
    recon = torch.empty(Wn, 1, HW, HW, device=dev) if return_reconstructions else None
    pl = eng.plan(F, 1)
    for w0 in range(0, Wn, F):
        nw = min(F, Wn - w0)
        nat.check(L.vad_ae_windows_forward(
            pl.h, cache.data_ptr(), x.data_ptr(), N, window, stride, w0, nw, o["seq"][w0:].data_ptr(),
            o["err"][w0:].data_ptr(), o["mem"][w0:].data_ptr(), o["score"][w0:].data_ptr(),
            None if recon is None else recon[w0:].data_ptr(), stream))
    out = {
        "anomaly_scores": o["score"],
        "recon_errors": o["err"],
        "memory_scores": o["mem"],
        "sequence_features": o["seq"],
        "frame_features": cache_field(cache, N, "lat"),
        "window_starts": torch.arange(Wn, dtype=torch.int64) * stride,
    }
    if recon is not None:
        out["reconstructed"] = recon
    return out
