"""bbox score_video on the GPU: the windowed first layer reads the video in place, so every window must come out as
the clip path has it for the same frames stacked into a clip -- bit for bit at the same batch size (the same kernels
at the same M) -- and within test_bbox.py's clip-forward tolerances of the CPU oracle: scores and graphs rtol 1e-4 /
atol 1e-6, features rtol 1e-4 / atol 1e-5 at 64 x 64 (its reference and packing tests) and atol 1e-4 of their scale
at ragged frame sizes (its ragged-shape test)."""
import numpy as np
import pytest
import torch

from oracle import bbox_oracle as bo
from tests.test_bbox import make_bbox_model
from tests.test_color_ingest_gpu import camera, host_color
from vad_amd import _native as nat
from vad_amd import data

pytestmark = pytest.mark.gpu


def video(seed, N, H, W):
    return torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(seed))


def stack_windows(x, window, stride):
    """(N, 3, H, W) -> the clips (Wn, 3, T, H, W) of its full windows, and their starts."""
    starts = list(range(0, x.shape[0] - window + 1, stride))
    return torch.stack([x[s:s + window].permute(1, 0, 2, 3) for s in starts]).contiguous(), starts


def clip_path(m, clips, batch):
    """model(clips) at score_video's batch sizes -> (scores (Wn,), graphs, features)."""
    outs = []
    with torch.no_grad():
        for w0 in range(0, clips.shape[0], batch):
            s, adj, f = m(clips[w0:w0 + batch].cuda())
            outs.append((s.reshape(-1).clone(), adj.clone(), f.clone()))
    return [torch.cat(t) for t in zip(*outs)]


def assert_oracle(o, seed, clips, ragged):
    p = {k: v.detach().cpu().clone() for k, v in make_bbox_model(dict(seed=seed)).state_dict().items()}
    with torch.no_grad():
        rs, radj, rf = bo.bbox_forward(p, clips)
    f_atol = 1e-4 * float(rf.abs().max()) if ragged else 1e-5
    np.testing.assert_allclose(o["anomaly_scores"].cpu().numpy(), rs.reshape(-1).numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(o["causal_graphs"].cpu().numpy(), radj.numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(o["features"].cpu().numpy(), rf.numpy(), rtol=1e-4, atol=f_atol)


def assert_is_clip_path(m, o, clips, starts, batch):
    Wn = len(starts)
    assert o["anomaly_scores"].shape == (Wn,) and o["causal_graphs"].shape == (Wn, 16, 16)
    assert o["features"].shape == (Wn, 1024)
    assert o["window_starts"].dtype == torch.int64 and o["window_starts"].tolist() == starts
    s, adj, f = clip_path(m, clips, batch)
    assert torch.equal(o["anomaly_scores"], s), "scores"
    assert torch.equal(o["causal_graphs"], adj), "graphs"
    assert torch.equal(o["features"], f), "features"


CASES = [
    # N, window, stride, batch, H, W
    (16, 8, 4, 3, 64, 64),    # one batch of three
    (8, 4, 4, 2, 20, 28),     # partial 8 x 8 pooled tiles in both directions (pooled 10 x 14)
    (19, 8, 1, 4, 64, 64),    # 12 windows: later batches start at frames 4 and 8
    (19, 8, 1, 5, 64, 64),    # 5 + 5 + 2: the last batch on a plan of its own size, starting at frame 10
    (19, 8, 3, 4, 64, 64),    # the last window ends at frame 17 of 19
    (19, 8, 11, 4, 64, 64),   # a stride beyond the window: two windows, frames 8..10 in none
    (19, 8, 3, 3, 20, 28),    # 3 + 1 at a ragged frame size
]


@pytest.mark.parametrize("N, window, stride, batch, H, W", CASES,
                         ids=[f"N{c[0]}-T{c[1]}-s{c[2]}-b{c[3]}-{c[4]}x{c[5]}" for c in CASES])
def test_score_video_is_the_clip_path_and_matches_the_oracle(N, window, stride, batch, H, W):
    seed = 70
    m = make_bbox_model(dict(seed=seed)).cuda()
    x = video(N * 100 + stride, N, H, W)
    clips, starts = stack_windows(x, window, stride)
    o = m.score_video(x.cuda(), window=window, stride=stride, batch=batch)
    assert_is_clip_path(m, o, clips, starts, batch)
    assert_oracle(o, seed, clips, ragged=(H, W) != (64, 64))


def test_window_defaults_to_num_frames_and_stride_to_four():
    m = make_bbox_model(dict(seed=71)).cuda()
    x = video(1, 17, 16, 18).cuda()
    o = m.score_video(x)
    assert o["window_starts"].tolist() == [0, 4, 8]
    w = m.score_video(x, window=8, stride=4, batch=2)
    for k in ("anomaly_scores", "causal_graphs", "features"):
        assert torch.equal(o[k], w[k]), k


def test_a_nan_pixel_reaches_exactly_the_windows_that_hold_its_frame():
    m = make_bbox_model(dict(seed=72)).cuda()
    x = video(2, 19, 64, 64)
    x[10, 1, 31, 17] = float("nan")
    o = m.score_video(x.cuda(), window=8, stride=3, batch=4)  # windows at 0, 3, 6, 9
    holds = torch.tensor([s <= 10 < s + 8 for s in o["window_starts"].tolist()])
    assert holds.tolist() == [False, True, True, True]
    assert torch.equal(torch.isnan(o["anomaly_scores"]).cpu(), holds)
    assert torch.equal(torch.isnan(o["features"]).any(1).cpu(), holds)
    assert torch.equal(torch.isnan(o["causal_graphs"]).flatten(1).any(1).cpu(), holds)
    clean = x.clone()
    clean[10, 1, 31, 17] = 0.5
    c = m.score_video(clean.cuda(), window=8, stride=3, batch=4)
    for k in ("anomaly_scores", "causal_graphs", "features"):
        assert torch.equal(o[k][0], c[k][0]), k  # the window without the frame is untouched


def test_score_video_leaves_clip_forwards_undisturbed():
    m = make_bbox_model(dict(seed=73)).cuda()
    a = bo.synth_clips(73, 0, 0, 2, 8, 64, 64).cuda()
    b = bo.synth_clips(73, 0, 1, 3, 8, 64, 64).cuda()
    x = video(3, 16, 64, 64).cuda()

    def run(disturb):
        with torch.no_grad():
            ra = [t.clone() for t in m(a)]
            if disturb:  # batches of 2 and 1: the plan of `a`'s size is borrowed in between
                m.score_video(x, batch=2)
            rb = [t.clone() for t in m(b)]
        return ra + rb

    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    quiet, got = run(False), run(True)
    for i, (g, q) in enumerate(zip(got, quiet)):
        assert torch.equal(g, q), i
    for k, v in m.state_dict().items():
        assert torch.equal(v, state[k]), f"{k} changed"


def test_im2col_path_scores_the_same_windows():
    """The knob bbox_im2col runs the windows through im2col3d on a strided view of the video: equal to the fused path
    within the 1e-5 test_bbox.py allows between the two paths."""
    m = make_bbox_model(dict(seed=74)).cuda()
    x = video(4, 11, 20, 28).cuda()
    o = m.score_video(x, window=4, stride=3, batch=2)
    nat.check(nat.lib().vad_set_tuning(b"bbox_im2col", 1))
    try:
        i = m.score_video(x, window=4, stride=3, batch=2)
    finally:
        nat.check(nat.lib().vad_set_tuning(b"bbox_im2col", 0))
    scale = float(o["features"].abs().max())
    np.testing.assert_allclose(i["features"].cpu().numpy(), o["features"].cpu().numpy(), rtol=1e-5, atol=1e-5 * scale)
    np.testing.assert_allclose(i["anomaly_scores"].cpu().numpy(), o["anomaly_scores"].cpu().numpy(), rtol=1e-4,
                               atol=1e-6)


def test_colour_route_from_camera_bytes():
    m = make_bbox_model(dict(seed=75)).cuda()
    u8 = camera(5, 16, 48, 80, "bgr")
    host = torch.from_numpy(host_color(u8, "bgr", (64, 64), 1, 3)).cuda()
    dev = data.ingest_u8(torch.from_numpy(u8).pin_memory(), (64, 64), 1, color="bgr", planes=3)
    assert torch.equal(dev, host)
    got, want = m.score_video(dev), m.score_video(host)
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_extract_anomalous_frames(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from vad_amd.bbox import AnomalyVisualizer
    rng = np.random.default_rng(6)
    sizes = [(48, 80), (30, 50), (64, 64), (71, 33)]
    decoded = {}
    for name, n in (("v1_short", 7), ("v2", 16), ("v3", 17)):
        (tmp_path / name).mkdir()
        for i in range(n):
            hs, ws = sizes[i % len(sizes)]
            rgb = rng.integers(0, 256, (hs, ws, 3), dtype=np.uint8)
            path = tmp_path / name / f"frame_{i:03d}.png"
            Image.fromarray(rgb).save(path)
            decoded[path] = rgb  # (PNG is lossless: what PIL decodes)
    (tmp_path / "notes.txt").write_text("not a folder")
    vis = AnomalyVisualizer(None, device="cuda")
    vis.model = make_bbox_model(dict(seed=76)).cuda()
    every = vis.extract_anomalous_frames(tmp_path, threshold=-1.0)
    assert [(c["video_id"], c["start_frame"]) for c in every] == [("v2", 0), ("v2", 4), ("v3", 0), ("v3", 4), ("v3", 8)]
    clips = []
    for c in every:
        assert set(c) == {"video_id", "start_frame", "end_frame", "frame_paths", "anomaly_score", "causal_graph",
                          "features"}
        assert c["end_frame"] == c["start_frame"] + 8
        want_paths = sorted((tmp_path / c["video_id"]).glob("*.png"))[c["start_frame"]:c["end_frame"]]
        assert list(c["frame_paths"]) == want_paths and len(want_paths) == 8
        assert isinstance(c["anomaly_score"], float)
        assert c["causal_graph"].shape == (16, 16) and c["features"].shape == (1024,)
        frames = [host_color(decoded[p][None], "rgb", (64, 64), 1, 3)[0] for p in want_paths]
        clips.append(np.stack(frames, axis=1))  # (3, 8, 64, 64)
    for c, (s, adj, f) in zip(every, vis.predict_clips(clips)):
        assert c["anomaly_score"] == pytest.approx(s, rel=1e-4, abs=1e-6)
        np.testing.assert_allclose(c["causal_graph"], adj, rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(c["features"], f, rtol=1e-4, atol=1e-5)
    # the threshold is strict: a clip's own score leaves it out
    scores = sorted(c["anomaly_score"] for c in every)
    assert len(set(scores)) == 5
    above = vis.extract_anomalous_frames(str(tmp_path), threshold=scores[2])
    assert sorted(c["anomaly_score"] for c in above) == scores[3:]
    assert vis.extract_anomalous_frames(tmp_path / "missing") == []
