"""Evaluation helpers: clip -> frame score broadcast and ROC-AUC, as the reference computes them
on the host (causal_anomaly_detection.py:1234-1251 `roc_auc_score(test_labels, test_scores)`, minicausal:374-390).

Every model in the reference scores whole clips; "frame-AUC" broadcasts each clip's score and label to its T
frames.  With equal-length clips that leaves the AUC unchanged (every clip is replicated T times), so frame-AUC ==
clip-AUC; with mixed T (config 5) the broadcast weights clips by length.  ``roc_auc`` is the Mann-Whitney
statistic with mid-ranks for ties, i.e. sklearn.metrics.roc_auc_score for binary labels.
"""
from __future__ import annotations

import numpy as np


def frame_scores(clip_scores, clip_lengths) -> np.ndarray:
    """Per-frame scores: clip i's score repeated clip_lengths[i] times (an int broadcasts to every clip)."""
    s = np.asarray(clip_scores, dtype=np.float64).reshape(-1)
    n = np.broadcast_to(np.asarray(clip_lengths, dtype=np.int64), s.shape)
    return np.repeat(s, n)


def window_frame_scores(window_scores, window_starts, window: int, n_frames: int) -> np.ndarray:
    """Per-frame curve of sliding-window scores (CausalAnomalyDetector.score_video): a frame's score is the mean over
    the windows [start, start + window) that cover it; a frame no window covers (a gap between windows when the stride
    exceeds the window, the trailing frames that fill no window) takes the score of the nearest covered frame, the
    earlier one on a tie.  For non-overlapping windows that tile the video this is ``frame_scores(scores, window)``."""
    s = np.asarray(window_scores, dtype=np.float64).reshape(-1)
    st = np.asarray(window_starts, dtype=np.int64).reshape(-1)
    if s.shape != st.shape or s.size == 0:
        raise ValueError("window_frame_scores: one start per score, at least one window")
    if window < 1 or n_frames < 1 or st.min() < 0 or st.max() + window > n_frames:
        raise ValueError("window_frame_scores: every window must lie inside [0, n_frames)")
    tot = np.zeros(n_frames, dtype=np.float64)
    cnt = np.zeros(n_frames, dtype=np.int64)
    for v, a in zip(s, st):  # (ascending window order: the same sum for every caller)
        tot[a:a + window] += v
        cnt[a:a + window] += 1
    covered = np.flatnonzero(cnt > 0)
    out = np.empty(n_frames, dtype=np.float64)
    out[covered] = tot[covered] / cnt[covered]
    for f in np.flatnonzero(cnt == 0):
        out[f] = out[covered[np.argmin(np.abs(covered - f))]]  # (argmin: the first, i.e. earlier, of two equally near)
    return out


def roc_auc(scores, labels) -> float:
    """Binary ROC-AUC (mid-ranks for tied scores).  Raises ValueError when only one class is present, as
    roc_auc_score does."""
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    y = np.asarray(labels).reshape(-1).astype(bool)
    npos, nneg = int(y.sum()), int((~y).sum())
    if npos == 0 or nneg == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    order = np.argsort(s, kind="mergesort")
    ranks = np.empty(len(s), dtype=np.float64)
    ss = s[order]
    i = 0
    while i < len(ss):  # mid-ranks over runs of equal scores
        j = i
        while j + 1 < len(ss) and ss[j + 1] == ss[i]:
            j += 1
        ranks[order[i:j + 1]] = 0.5 * (i + j) + 1.0
        i = j + 1
    u = ranks[y].sum() - npos * (npos + 1) / 2.0
    return float(u / (npos * nneg))


def frame_auc(clip_scores, clip_labels, clip_lengths) -> float:
    """Frame-level AUC of clip scores and clip labels broadcast to their frames."""
    return roc_auc(frame_scores(clip_scores, clip_lengths), frame_scores(clip_labels, clip_lengths))


def evaluate_auc(model, loader) -> tuple[float, np.ndarray, np.ndarray]:
    """Scores every clip of ``loader`` with the HIP model (eval mode) and returns (frame-AUC, scores, labels), the
    quantity the reference prints after test_model (cad:1234-1251)."""
    from .train import test_model
    scores, labels, outs = test_model(model, loader)
    lengths = [len(per_clip) for o in outs for per_clip in o["detections"]]  # T frames per clip
    return frame_auc(scores, labels, lengths), np.asarray(scores), np.asarray(labels)
