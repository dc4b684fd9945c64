"""CausalAnomalyDetector.score_video on the GPU against the CPU oracle: window w of the video must equal the oracle's
eval forward of the clip frames[w * stride : w * stride + T] at clip index clip0 + w (oracle.cad_oracle.cad_forward on
the stacked windows), at the project's forward tolerance rtol 1e-4 / atol 1e-5; box counts and Nmax must be equal."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import cad_oracle as co
from tests.golden.cases import FORCED_A
from tests.golden_util import make_cad_model

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-4, atol=1e-5)
# validity thresholds of the decoded boxes (cad:217-218), per coordinate (x, y, w, h)
THRESHOLDS = {0: (10.0, 350.0), 1: (10.0, 230.0), 2: (10.0, 100.0), 3: (20.0, 150.0)}


def _oracle_windows(case, frames, T, stride, seed, step, clip0):
    """The yardstick: the oracle's eval forward on the stacked windows."""
    sd = {k: v.clone() for k, v in make_cad_model(case).state_dict().items()}
    params = {k: v for k, v in sd.items() if "running" not in k and "num_batches" not in k}
    bufs = {k: v for k, v in sd.items() if "running" in k}
    Wn = (frames.shape[0] - T) // stride + 1
    X = torch.stack([frames[w * stride:w * stride + T] for w in range(Wn)])
    with torch.no_grad():
        return co.cad_forward(params, bufs, X, co.CadDraws.make(seed, step, clip0, Wn, T), training=False)


def _check_against_oracle(out, ref, N, T, stride, tol=None):
    """tol: {output key: dict(rtol=, atol=)} replacing TOL for that key ("detections", "causal_factors" and the five
    stacked outputs); the keys it leaves out keep TOL."""
    tol = tol or {}
    Wn = (N - T) // stride + 1
    assert out["window_starts"].tolist() == [w * stride for w in range(Wn)]
    # counts first: a wrong count makes every later comparison meaningless
    ref_det = {}
    for w in range(Wn):
        for t in range(T):
            ref_det[w * stride + t] = ref["detections"][w][t]
    assert len(out["detections"]) == N
    for f, d in ref_det.items():
        got = out["detections"][f].cpu().numpy()
        assert got.shape == tuple(d.shape), f"frame {f}: {got.shape[0]} boxes, oracle {d.shape[0]}"
        np.testing.assert_allclose(got, d.numpy(), err_msg=f"boxes of frame {f}", **tol.get("detections", TOL))
    ref_nmax = [z.shape[0] for z in ref["causal_factors"]]
    assert [z.shape[0] for z in out["causal_factors"]] == ref_nmax
    np.testing.assert_allclose(out["anomaly_scores"].cpu().numpy(), ref["anomaly_scores"].numpy(),
                               **tol.get("anomaly_scores", TOL))
    np.testing.assert_allclose(out["direct_predictions"].cpu().numpy(), ref["direct_predictions"].numpy(),
                               **tol.get("direct_predictions", TOL))
    np.testing.assert_allclose(out["causal_anomaly_scores"].cpu().numpy(), ref["causal_anomaly_scores"].numpy(),
                               **tol.get("causal_anomaly_scores", TOL))
    np.testing.assert_allclose(out["kl_losses"].cpu().numpy(), torch.stack(ref["kl_losses"]).numpy(),
                               **tol.get("kl_losses", TOL))
    np.testing.assert_allclose(out["adjacency_matrices"].cpu().numpy(), torch.stack(ref["adjacency_matrices"]).numpy(),
                               **tol.get("adjacency_matrices", TOL))
    for w in range(Wn):
        np.testing.assert_allclose(out["causal_factors"][w].cpu().numpy(), ref["causal_factors"][w].numpy(),
                                   err_msg=f"z of window {w}", **tol.get("causal_factors", TOL))
    return ref_nmax


def test_fallback_ragged_chunks_windows_across_seams():
    """Reference init (every frame takes the fallback box), N = 11 in chunks of 4, 4, 3; 8 windows of 4 at stride 1,
    most of them across a chunk seam; seed 7 / clip0 3 so that a wrong key of the VAE noise shows."""
    case = dict(name="sv_fallback", seed=0, forced=None)
    N, T, stride, H, W = 11, 4, 1, 64, 64
    frames = co.synth_clips(0, 0, 0, 1, N, H, W)[0]
    ref = _oracle_windows(case, frames, T, stride, 7, 0, 3)
    m = make_cad_model(case).cuda().eval()
    out = m.score_video(frames.cuda(), window=T, stride=stride, chunk=4, seed=7, clip0=3)
    assert out["anomaly_scores"].shape == (8,)
    assert _check_against_oracle(out, ref, N, T, stride) == [1] * 8
    # the (1, N, 1, H, W) form is the same video
    out5 = m.score_video(frames.cuda()[None], window=T, stride=stride, chunk=4, seed=7, clip0=3)
    assert torch.equal(out5["anomaly_scores"], out["anomaly_scores"])


# Model and frame seed of the forced case.  Seeds 1..20 (model seed x frame seed, all 400 pairs) give every frame of
# the video the same box count with the oracle -- synthetic noise frames move the decoded boxes by hundredths of a
# pixel -- so no window differs in Nmax; scanning on with the oracle alone (model seed = frame seed), 130 is the first
# seed that meets all three fixture conditions: counts [4]*11 + [5, 4], Nmax [4, 4, 4, 4, 5], margin 1.75e-3 px.
FORCED_SEED = 130


@pytest.fixture(scope="module")
def forced_video():
    case = dict(name="sv_forced", seed=FORCED_SEED, forced=FORCED_A)
    N, H, W = 13, 96, 80
    frames = co.synth_clips(FORCED_SEED, 0, 0, 1, N, H, W)[0]
    return case, frames


@pytest.mark.parametrize("stride, starts", [(2, [0, 2, 4, 6, 8]), (3, [0, 3, 6])])
def test_forced_detections_window_dependent_nmax(forced_video, stride, starts):
    """FORCED_A at 96x80, N = 13, T = 5, chunks of 6, 6, 1.  stride 2: five windows, Nmax differs between windows.
    stride 3 (same model and frames): three windows and two trailing frames, which get detections but no score."""
    case, frames = forced_video
    N, T = 13, 5
    ref = _oracle_windows(case, frames, T, stride, 11, 2, 5)
    ref_nmax = [z.shape[0] for z in ref["causal_factors"]]
    if stride == 2:
        assert max(ref_nmax) >= 2, f"fixture, not kernel: no window of the oracle has two trajectories ({ref_nmax})"
        assert len(set(ref_nmax)) >= 2, f"fixture, not kernel: every window of the oracle has Nmax {ref_nmax[0]}"
    boxes = ref["boxes"].numpy()
    margin = min(float(np.abs(boxes[..., q] - t).min()) for q, ts in THRESHOLDS.items() for t in ts)
    assert margin >= 1e-3, f"fixture, not kernel: an oracle box coordinate lies {margin:.3g} px from a threshold"
    m = make_cad_model(case).cuda().eval()
    out = m.score_video(frames.cuda(), window=T, stride=stride, chunk=6, seed=11, step=2, clip0=5)
    assert out["window_starts"].tolist() == starts
    assert _check_against_oracle(out, ref, N, T, stride) == ref_nmax
    if stride == 3:  # frames 11, 12 fill no window: their detections against the oracle's frame-by-frame clip
        tail = _oracle_windows(case, frames[11:], 1, 1, 0, 0, 0)
        for i, f in enumerate((11, 12)):
            np.testing.assert_allclose(out["detections"][f].cpu().numpy(), tail["detections"][i][0].numpy(), **TOL)


def test_single_frame_windows():
    """T = 1: a one-step recurrence and a mean over one frame (N = 3, stride 1, forced, 64x64)."""
    case = dict(name="sv_t1", seed=5, forced=FORCED_A)
    N, T, H, W = 3, 1, 64, 64
    frames = co.synth_clips(5, 0, 0, 1, N, H, W)[0]
    ref = _oracle_windows(case, frames, T, 1, 2, 1, 0)
    m = make_cad_model(case).cuda().eval()
    out = m.score_video(frames.cuda(), window=1, stride=1, seed=2, step=1)
    _check_against_oracle(out, ref, N, T, 1)


@pytest.mark.parametrize("forced", [None, FORCED_A], ids=["fallback", "forced"])
def test_agrees_with_the_clip_forward(forced):
    """stride = T = 4, N = 8: the windows are the clips of m(X); every output within 1e-6 absolute of the clip path on
    the same device."""
    case = dict(name="sv_clip", seed=1, forced=forced)
    N, T, H, W = 8, 4, 64, 64
    frames = co.synth_clips(1, 0, 0, 1, N, H, W)[0].cuda()
    m = make_cad_model(case).cuda().eval()
    with torch.no_grad():
        clip = m(frames.view(2, T, 1, H, W), seed=9, step=1, clip0=2)
    out = m.score_video(frames, window=T, stride=T, seed=9, step=1, clip0=2)
    pairs = [("anomaly_scores", out["anomaly_scores"], clip["anomaly_scores"]),
             ("direct_predictions", out["direct_predictions"], clip["direct_predictions"]),
             ("causal_anomaly_scores", out["causal_anomaly_scores"], clip["causal_anomaly_scores"]),
             ("kl_losses", out["kl_losses"], torch.stack(clip["kl_losses"])),
             ("adjacency_matrices", out["adjacency_matrices"], torch.stack(clip["adjacency_matrices"]))]
    for b in range(2):
        pairs.append((f"causal_factors[{b}]", out["causal_factors"][b], clip["causal_factors"][b]))
        for t in range(T):
            pairs.append((f"detections[{b}][{t}]", out["detections"][b * T + t], clip["detections"][b][t]))
    worst, identical = 0.0, True
    for name, a, c in pairs:
        assert a.shape == c.shape, name
        d = float((a - c).abs().max()) if a.numel() else 0.0
        worst = max(worst, d)
        identical = identical and torch.equal(a, c)
        assert d <= 1e-6, f"{name}: {d:.3g} from the clip path"
    print(f"score_video vs clip forward ({'forced' if forced else 'fallback'}): max abs diff {worst:.3g}, "
          f"bit-identical: {identical}")


def test_no_side_effects_and_stale_backward_raises():
    case = dict(name="sv_side", seed=2, forced=FORCED_A)
    T, H, W = 4, 64, 64
    m = make_cad_model(case).cuda().eval()
    x = co.synth_clips(2, 0, 0, 2, T, H, W).cuda()
    frames = co.synth_clips(3, 0, 0, 1, 6, H, W)[0].cuda()
    before = m(x, seed=4)
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    pending = m(x, seed=4)["anomaly_scores"].sum()
    m.score_video(frames, window=T, stride=1, chunk=4)
    for k, v in m.state_dict().items():
        assert torch.equal(v, state[k]), f"{k} changed"
    assert any(k.endswith("num_batches_tracked") for k in state) and any("running_var" in k for k in state)
    with pytest.raises(RuntimeError, match="most recent forward only"):
        pending.backward()
    after = m(x, seed=4)
    for k in ("anomaly_scores", "direct_predictions", "causal_anomaly_scores"):
        assert torch.equal(before[k], after[k]), k
    for a, b in zip(before["causal_factors"] + before["adjacency_matrices"] + before["kl_losses"],
                    after["causal_factors"] + after["adjacency_matrices"] + after["kl_losses"]):
        assert torch.equal(a, b)
    for da, db in zip(before["detections"], after["detections"]):
        for a, b in zip(da, db):
            assert torch.equal(a, b)


def test_abi_errors_launch_nothing():
    """T > nframes, stride = 0 and a window range past the end: non-zero, a message that names the argument, and the
    prefilled outputs untouched."""
    from vad_amd import _native as nat
    L = nat.lib()
    case = dict(name="sv_abi", seed=0, forced=None)
    m = make_cad_model(case).cuda().eval()
    N, T, H, W = 6, 4, 64, 64
    frames = co.synth_clips(0, 0, 0, 1, N, H, W)[0].cuda()
    m.score_video(frames, window=T, chunk=N)  # builds and binds the (N, 1, H, W) plan
    pl = m.engine().plan(N, 1, H, W)
    dev = frames.device
    cache = torch.zeros(L.vad_cad_frame_cache_floats(N), device=dev)
    outs = [torch.full((N * k,), 7.0, device=dev) for k in (1, 2, 1, 1, 30, 36)]
    nmax = torch.full((N,), 7, dtype=torch.int32, device=dev)

    def call(T_, stride, w0, nw):
        return L.vad_cad_windows_forward(pl.h, cache.data_ptr(), N, T_, stride, w0, nw, 0, 0, 0,
                                         *[o.data_ptr() for o in outs], nmax.data_ptr(), nat.stream_of(dev))

    for args, text in [((N + 1, 1, 0, 1), b"T must be in 1..nframes"),
                       ((T, 0, 0, 1), b"stride must be >= 1"),
                       ((T, 1, 2, 2), b"w0 .. w0 + nw - 1 reach outside the video")]:
        assert call(*args) != 0
        assert text in L.vad_last_error(), L.vad_last_error()
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == 7.0).all())
    assert bool((nmax == 7).all())
    assert L.vad_cad_frames_forward(pl.h, frames.data_ptr(), N, cache.data_ptr(), 1, nat.stream_of(dev)) != 0
    assert b"outside the nframes of the cache" in L.vad_last_error()
    assert call(T, 1, 0, 3) == 0  # and the same call with legal arguments runs
    torch.cuda.synchronize()
    assert bool((nmax[:3] == 1).all()) and bool((nmax[3:] == 7).all())
