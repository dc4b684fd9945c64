"""VideoAutoEncoder.score_video without a device: the argument checks raise before any device work, and one
window_frame_scores case of the reference's own stride (T // 4, cad1:72) that tests/test_score_video.py lacks."""
import numpy as np
import pytest
import torch

from vad_amd import evaluate as ev
from vad_amd.ae import VideoAutoEncoder


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return VideoAutoEncoder().eval()


@pytest.mark.parametrize("frames, kw, text", [
    (torch.zeros(8, 1, 64, 64), dict(window=9), "fewer than one window"),
    (torch.zeros(8, 1, 64, 64), dict(window=4, stride=0), "stride"),
    (torch.zeros(8, 1, 64, 64), dict(window=4, stride=1.5), "stride"),
    (torch.zeros(8, 1, 64, 64), dict(window=4, chunk=0), "chunk"),
    (torch.zeros(8, 1, 64, 64), dict(window=0), "window"),
    (torch.zeros(8, 1, 64, 64), dict(window=-2), "window"),
    (torch.zeros(8, 64, 64), dict(window=4), r"\(N, 1, 64, 64\)"),
    (torch.zeros(8, 1, 32, 32), dict(window=4), r"\(N, 1, 64, 64\)"),
    (torch.zeros(8, 3, 64, 64), dict(window=4), r"\(N, 1, 64, 64\)"),
    (torch.zeros(1, 8, 1, 64, 32), dict(window=4), r"\(N, 1, 64, 64\)"),
    (torch.zeros(2, 8, 1, 64, 64), dict(window=4), "one video per call"),
    ([[0.0]], dict(window=1), r"\(N, 1, 64, 64\)"),
])
def test_score_video_rejects_bad_arguments_without_a_device(model, frames, kw, text):
    with pytest.raises(ValueError, match=text):
        model.score_video(frames, **kw)


def test_score_video_rejects_training_mode(model):
    model.train()
    try:
        with pytest.raises(ValueError, match="eval mode"):
            model.score_video(torch.zeros(8, 1, 64, 64), window=4)
    finally:
        model.eval()


def test_legal_arguments_reach_the_device_check(model):
    """Every argument legal on a CPU model: the first thing to fail is the device requirement, not a ValueError."""
    with pytest.raises(RuntimeError, match="HIP"):
        model.score_video(torch.zeros(1, 8, 1, 64, 64), window=4, stride=2, chunk=3)


def test_window_frame_scores_at_the_reference_stride():
    # window 8 at the reference's stride T // 4 = 2 over 13 frames: starts 0, 2, 4 cover frames 0..11; frame f lies in
    # the windows w with 2w <= f <= 2w + 7, the uncovered frame 12 takes frame 11's value
    s = [1.0, 2.0, 4.0]
    got = ev.window_frame_scores(s, [0, 2, 4], 8, 13)
    want = [1, 1, 1.5, 1.5] + [7 / 3] * 4 + [3, 3, 4, 4, 4]
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-15)
