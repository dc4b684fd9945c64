"""CausalAnomalyDetector.score_video and evaluate.window_frame_scores without a device: the argument checks raise
before any device work, and the per-frame curve matches hand-computed tables."""
import numpy as np
import pytest
import torch

from vad_amd import evaluate as ev
from vad_amd.cad import CausalAnomalyDetector


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return CausalAnomalyDetector().eval()


@pytest.mark.parametrize("frames, kw, text", [
    (torch.zeros(8, 1, 32, 32), dict(window=9), "fewer than one window"),
    (torch.zeros(8, 1, 32, 32), dict(window=4, stride=0), "stride"),
    (torch.zeros(8, 1, 32, 32), dict(window=4, chunk=0), "chunk"),
    (torch.zeros(8, 1, 32, 32), dict(window=0), "window"),
    (torch.zeros(8, 32, 32), dict(window=4), "shape"),
    (torch.zeros(2, 8, 1, 32, 32), dict(window=4), "one video per call"),
    (torch.zeros(8, 3, 32, 32), dict(window=4), "single-channel"),
])
def test_score_video_rejects_bad_arguments_without_a_device(model, frames, kw, text):
    with pytest.raises(ValueError, match=text):
        model.score_video(frames, **kw)


def test_score_video_rejects_training_mode_and_bf16(model):
    x = torch.zeros(8, 1, 32, 32)
    model.train()
    try:
        with pytest.raises(ValueError, match="eval mode"):
            model.score_video(x, window=4)
    finally:
        model.eval()
    model.set_compute_dtype(torch.bfloat16)
    try:
        with pytest.raises(ValueError, match="fp32 only"):
            model.score_video(x, window=4)
    finally:
        model.set_compute_dtype(torch.float32)


def test_window_frame_scores_stride_one():
    # windows of 3 at starts 0..3 over 6 frames: frame f is covered by windows max(0, f-2) .. min(3, f)
    s = [1.0, 2.0, 4.0, 8.0]
    got = ev.window_frame_scores(s, [0, 1, 2, 3], 3, 6)
    want = [1.0, (1 + 2) / 2, (1 + 2 + 4) / 3, (2 + 4 + 8) / 3, (4 + 8) / 2, 8.0]
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-15)


def test_window_frame_scores_stride_equal_to_window_is_the_clip_broadcast():
    s = [0.25, 0.5, 0.125]
    got = ev.window_frame_scores(torch.tensor(s), torch.tensor([0, 4, 8]), 4, 12)
    np.testing.assert_array_equal(got, ev.frame_scores(s, 4))


def test_window_frame_scores_uncovered_frames_take_the_nearest_covered():
    # window 3, stride 5 over 13 frames: windows at 0 and 5 cover 0-2 and 5-7; 3 -> 2, 4 -> 5, 8.. -> 7
    got = ev.window_frame_scores([1.0, 3.0], [0, 5], 3, 13)
    np.testing.assert_array_equal(got, [1, 1, 1, 1, 3, 3, 3, 3, 3, 3, 3, 3, 3])
    # a tie (frame 3 between covered frames 2 and 4) goes to the earlier frame
    got = ev.window_frame_scores([1.0, 3.0], [0, 4], 3, 7)
    np.testing.assert_array_equal(got, [1, 1, 1, 1, 3, 3, 3])
    # trailing frames of a stride-2 sweep: N = 8, window 3 -> starts 0, 2, 4; frame 7 is covered by no window
    got = ev.window_frame_scores([1.0, 2.0, 4.0], [0, 2, 4], 3, 8)
    np.testing.assert_allclose(got, [1, 1, 1.5, 2, 3, 4, 4, 4], rtol=0, atol=1e-15)


def test_window_frame_scores_rejects_windows_outside_the_video():
    with pytest.raises(ValueError):
        ev.window_frame_scores([1.0], [6], 3, 8)
    with pytest.raises(ValueError):
        ev.window_frame_scores([1.0, 2.0], [0], 3, 8)
