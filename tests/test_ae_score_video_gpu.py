"""VideoAutoEncoder.score_video on the GPU against the CPU oracle: window w of the video must equal the oracle's eval
batch on the clip frames[w * stride : w * stride + T] (oracle.ae_oracle.ae_eval_batch on the stacked windows), at the
project's tolerances for this model's forward (tests/test_ae_gpu.py): rtol 1e-4 / atol 1e-5 on features, memory scores
and combined scores, rtol 1e-4 / atol 1e-6 on reconstruction errors.

Two fixture conditions, asserted from the oracle alone: the BatchNorm running statistics are perturbed (at init they
are mean 0 / variance 1, which a kernel that ignored them would pass), and every frame has structure of its own, so
that adjacent windows differ in every compared output by at least 10x its tolerance (pure noise frames give windows
whose errors differ by less than the tolerance: an off-by-one window start would pass)."""
import numpy as np
import pytest
import torch

from oracle import ae_oracle as ae
from tests.test_ae_oracle import make_ae_model

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-4, atol=1e-5)
TOL_ERR = dict(rtol=1e-4, atol=1e-6)
HW = 64


def make_frames(seed, N):
    """(N, 1, 64, 64): half noise, half a per-frame grey level rising over the video, times a column ramp whose
    exponent cycles with the frame index, clamped as the reference's loader does (cad1:110-114)."""
    noise = ae.synth_clips(seed, 0, 0, 1, N)[0]
    level = torch.linspace(0.15, 0.85, N).view(N, 1, 1, 1)
    ramp = torch.linspace(0.3, 1.0, HW).view(1, 1, 1, HW) ** (torch.arange(N) % 3).view(N, 1, 1, 1).float()
    return torch.clamp((0.5 * noise + 0.5 * level) * ramp, 0.001, 0.999)


def make_model(seed, mem=(30, 30)):
    """The drop-in module (reference init under the seed, the ring state of the existing eval case) with every BN
    running mean overwritten by seeded values in +-0.1 and every running variance by values in [0.5, 1.5]."""
    m = make_ae_model(dict(seed=seed, mem=mem))
    g = torch.Generator().manual_seed(1000 + seed)
    with torch.no_grad():
        for k, v in m.state_dict().items():
            if k.endswith("running_mean"):
                v.copy_((torch.rand(v.shape, generator=g) * 2 - 1) * 0.1)
            elif k.endswith("running_var"):
                v.copy_(0.5 + torch.rand(v.shape, generator=g))
    return m.eval()


def stack_windows(frames, T, stride):
    Wn = (frames.shape[0] - T) // stride + 1
    return torch.stack([frames[w * stride:w * stride + T] for w in range(Wn)])


def oracle_windows(m, frames, T, stride):
    """The yardstick: the oracle's eval batch on the stacked windows, from the CPU module's own state."""
    params, bufs, mem = ae.split_state(m.state_dict())
    for k, v in bufs.items():
        init = torch.zeros_like(v) if k.endswith("running_mean") else torch.ones_like(v)
        assert float((v - init).abs().max()) > 0.01, f"fixture, not kernel: {k} is still at its initial value"
    ref = ae.ae_eval_batch(params, bufs, mem, stack_windows(frames, T, stride))
    ref["state"] = (params, bufs, mem)
    return ref


def ref_outputs(ref):
    o = ref["outputs"]
    return {"anomaly_scores": (ref["combined"], TOL), "recon_errors": (ref["recon_error"], TOL_ERR),
            "memory_scores": (o["anomaly_score"], TOL), "sequence_features": (o["sequence_feature"], TOL)}


def assert_windows_differ(ref, keys):
    """Adjacent oracle windows differ in every compared output by at least 10x the tolerance it is compared at."""
    for k in keys:
        v, tol = ref_outputs(ref)[k]
        v = v.reshape(v.shape[0], -1).double()
        for w in range(v.shape[0] - 1):
            d = float((v[w + 1] - v[w]).abs().max())
            need = 10 * (tol["atol"] + tol["rtol"] * float(torch.maximum(v[w].abs(), v[w + 1].abs()).max()))
            assert d >= need, (f"fixture, not kernel: {k} of oracle windows {w} and {w + 1} differ by {d:.3g}, "
                               f"less than 10x the tolerance ({need:.3g})")


def check_against_oracle(out, ref, N, T, stride, keys):
    Wn = (N - T) // stride + 1
    assert out["window_starts"].tolist() == [w * stride for w in range(Wn)]
    assert out["window_starts"].dtype == torch.int64 and out["window_starts"].device.type == "cpu"
    for k in ("anomaly_scores", "recon_errors", "memory_scores"):
        assert out[k].shape == (Wn,), k
    assert out["sequence_features"].shape == (Wn, 64) and out["frame_features"].shape == (N, 64)
    for k in keys:
        v, tol = ref_outputs(ref)[k]
        np.testing.assert_allclose(out[k].cpu().numpy(), v.numpy(), err_msg=k, **tol)
    ff = out["frame_features"].cpu().numpy()
    rff = ref["outputs"]["frame_features"].numpy()
    for w in range(Wn):
        for t in range(T):
            np.testing.assert_allclose(ff[w * stride + t], rff[w, t], err_msg=f"frame {w * stride + t}", **TOL)
    if "reconstructed" in out:
        assert out["reconstructed"].shape == (Wn, 1, HW, HW)
        np.testing.assert_allclose(out["reconstructed"].cpu().numpy(), ref["outputs"]["reconstructed"][:, 0].numpy(),
                                   err_msg="reconstructed", **TOL)


ALL = ("anomaly_scores", "recon_errors", "memory_scores", "sequence_features")


@pytest.fixture(scope="module")
def seam_case():
    """N = 11, T = 4, stride 1 with the ring filled: model, frames and the oracle's windows, computed once."""
    m = make_model(46)
    frames = make_frames(3, 11)
    ref = oracle_windows(m, frames, 4, 1)
    assert_windows_differ(ref, ALL)
    return m, frames, ref


def test_seams_and_batches(seam_case):
    """Frame chunks of 4, 4, 3; the 8 windows in batches of 4 and 4, most of them across a chunk seam."""
    m, frames, ref = seam_case
    N, T = 11, 4
    md = make_model(46).cuda()
    out = md.score_video(frames.cuda(), window=T, stride=1, chunk=4, return_reconstructions=True)
    assert out["anomaly_scores"].shape == (8,)
    check_against_oracle(out, ref, N, T, 1, ALL)
    out5 = md.score_video(frames.cuda()[None], window=T, stride=1, chunk=4, return_reconstructions=True)
    assert set(out5) == set(out)
    for k in out:
        assert torch.equal(out5[k], out[k]), k
    assert "reconstructed" not in md.score_video(frames.cuda(), window=T, chunk=4)


def test_stride_trailing_frames_and_ragged_window_batch():
    """N = 13, T = 5, stride 3, chunks of 6, 6, 1: starts 0, 3, 6 -- three windows on a six-row plan; frames 11 and 12
    fill no window and get frame features, checked against the oracle's encoder, and no score."""
    N, T, stride = 13, 5, 3
    m = make_model(47)
    frames = make_frames(5, N)
    ref = oracle_windows(m, frames, T, stride)
    assert_windows_differ(ref, ALL)
    out = m.cuda().score_video(frames.cuda(), window=T, stride=stride, chunk=6, return_reconstructions=True)
    assert out["window_starts"].tolist() == [0, 3, 6]
    check_against_oracle(out, ref, N, T, stride, ALL)
    params, bufs, _ = ref["state"]
    with torch.no_grad():
        tail = ae.nan0(ae.encoder(params, bufs, frames[11:], False))
    assert float((tail[0] - tail[1]).abs().max()) >= 10 * (1e-5 + 1e-4 * float(tail.abs().max())), \
        "fixture, not kernel: the oracle's latents of frames 11 and 12 are too close to tell apart"
    np.testing.assert_allclose(out["frame_features"][11:].cpu().numpy(), tail.numpy(), **TOL)


def test_single_frame_windows():
    """T = 1, N = 3: a one-step recurrence, and the error against a single frame.  (Frame seed 8: with seed 7 the
    oracle's memory scores of windows 0 and 1 differ by 2.8e-4, under 10x their tolerance; chosen on the oracle
    alone.)"""
    N = 3
    m = make_model(48)
    frames = make_frames(8, N)
    ref = oracle_windows(m, frames, 1, 1)
    assert_windows_differ(ref, ALL)
    out = m.cuda().score_video(frames.cuda(), window=1, stride=1, return_reconstructions=True)
    check_against_oracle(out, ref, N, 1, 1, ALL)


def test_empty_ring_scores_zero():
    """memory_ptr = 9 over non-zero rows: memory scores exactly 0, combined = 0.7 * error."""
    N, T = 6, 3
    m = make_model(49, mem=(30, 9))
    assert int(m.memory_ptr) == 9 and float(m.normal_memory[:9].abs().min()) > 0, \
        "fixture, not kernel: the ring rows below the pointer must be non-zero"
    frames = make_frames(9, N)
    ref = oracle_windows(m, frames, T, 1)
    keys = ("anomaly_scores", "recon_errors", "sequence_features")
    assert_windows_differ(ref, keys)
    assert bool((ref["outputs"]["anomaly_score"] == 0).all()), "fixture, not kernel: the oracle's ring is not empty"
    out = m.cuda().score_video(frames.cuda(), window=T, stride=1)
    assert bool((out["memory_scores"] == 0).all())
    check_against_oracle(out, ref, N, T, 1, keys)
    np.testing.assert_allclose(out["anomaly_scores"].cpu().numpy(), 0.7 * out["recon_errors"].cpu().numpy(), **TOL)


def _clip_pairs(out, clip, T):
    B = clip["sequence_feature"].shape[0]
    pairs = [("sequence_feature", out["sequence_features"], clip["sequence_feature"]),
             ("frame_features", out["frame_features"], clip["frame_features"].reshape(B * T, 64)),
             ("anomaly_score", out["memory_scores"], clip["anomaly_score"]),
             ("recon_error", out["recon_errors"], clip["recon_error"]),
             ("combined", out["anomaly_scores"], 0.7 * clip["recon_error"] + 0.3 * clip["anomaly_score"])]
    for t in range(T):
        pairs.append((f"reconstructed[:, {t}]", out["reconstructed"], clip["reconstructed"][:, t]))
    return pairs


def test_agrees_with_the_clip_forward():
    """stride = T = 4, N = 8, chunk = 8: the windows are the clips of the eval batch; every output within 1e-6
    absolute of the clip path on the same device, the one decoded frame against each of the clip's T copies.

    On an MI355X the line printed below read "max abs diff 0, bit-identical: True" (quoted in DESIGN 2.2)."""
    N, T = 8, 4
    m = make_model(50).cuda()
    frames = make_frames(11, N).cuda()
    clip = m.engine().forward(frames.view(2, T, 1, HW, HW), stages=3, training=False, loss_mode=1)
    clip = {k: v.clone() for k, v in clip.items()}
    out = m.score_video(frames, window=T, stride=T, chunk=8, return_reconstructions=True)
    worst, identical = 0.0, True
    for name, a, c in _clip_pairs(out, clip, T):
        assert a.shape == c.shape, name
        d = float((a - c).abs().max())
        worst = max(worst, d)
        identical = identical and torch.equal(a, c)
        print(f"  {name}: max abs diff {d:.3g}")
    print(f"ae score_video vs clip forward: max abs diff {worst:.3g}, bit-identical: {identical}")
    for name, a, c in _clip_pairs(out, clip, T):
        d = float((a - c).abs().max())
        assert d <= 1e-6, f"{name}: {d:.3g} from the clip path"


def test_nan_pixels_are_zero_as_in_the_clip_path():
    """NaN pixels become 0 before the encoder and in the error, as AeTrainer.eval_batch treats them."""
    from vad_amd.ae import AeTrainer
    N, T = 8, 4
    m = make_model(51).cuda()
    frames = make_frames(13, N)
    frames[2, 0, 5, 7:40] = float("nan")
    frames[6, 0, 60, :] = float("nan")
    frames = frames.cuda()
    clip = AeTrainer(m).eval_batch(frames.view(2, T, 1, HW, HW))
    clip = {k: v.clone() for k, v in clip.items()}
    zeroed = AeTrainer(m).eval_batch(torch.nan_to_num(frames, nan=0.0).view(2, T, 1, HW, HW))
    assert torch.equal(zeroed["recon_error"], clip["recon_error"]) and bool(torch.isfinite(clip["recon_error"]).all())
    out = m.score_video(frames, window=T, stride=T, chunk=8, return_reconstructions=True)
    for name, a, c in _clip_pairs(out, clip, T):
        d = float((a - c).abs().max())
        assert d <= 1e-6, f"{name}: {d:.3g} from the clip path"


def test_no_side_effects_and_stale_backward_raises():
    from vad_amd.ae import AeTrainer
    F, T = 4, 4
    m, twin = make_model(52).cuda(), make_model(52).cuda()
    frames = make_frames(15, 7).cuda()
    clips = ae.synth_clips(52, 0, 0, 2, T).cuda()
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    for name in ("running_var", "num_batches_tracked", "normal_memory", "memory_ptr"):
        assert any(k.endswith(name) for k in state), name
    pending = m(frames[:F].view(F, 1, 1, HW, HW))["reconstructed"].sum()
    m.score_video(frames, window=T, stride=1, chunk=F)
    for k, v in m.state_dict().items():
        assert torch.equal(v, state[k]), f"{k} changed"
    with pytest.raises(RuntimeError, match="needs a preceding full forward"):
        pending.backward()
    la = AeTrainer(m, lr=1e-4).step(clips).clone()
    lb = AeTrainer(twin, lr=1e-4).step(clips).clone()
    assert float(la[3]) == 2.0 and torch.equal(la, lb)
    sa, sb = m.state_dict(), twin.state_dict()
    moved = 0
    for k in sa:
        assert torch.equal(sa[k], sb[k]), f"{k} differs from the twin that never called score_video"
        moved += int(not torch.equal(sa[k], state[k]))
    assert moved > 10  # the step did train


def test_abi_errors_launch_nothing():
    """Each bad argument: non-zero, a message that names it, and the prefilled outputs untouched."""
    from vad_amd import _native as nat
    L = nat.lib()
    N, T = 6, 4
    m = make_model(53).cuda()
    frames = make_frames(17, 2 * N).cuda()
    ref = m.score_video(frames[:N], window=T, chunk=N, return_reconstructions=True)  # binds the (N, 1) plan
    pl = m.engine().plan(N, 1)
    dev = frames.device
    st = nat.stream_of(dev)
    cache = torch.empty(L.vad_ae_frame_cache_floats(N), device=dev)
    assert cache.numel() == N * 320 and L.vad_ae_frame_cache_offset(N, 0) == 0
    assert L.vad_ae_frame_cache_offset(N, 1) == N * 64
    assert L.vad_ae_frame_cache_floats(0) == -1 and L.vad_ae_frame_cache_offset(N, 2) == -1
    assert L.vad_ae_frames_forward(pl.h, frames.data_ptr(), N, cache.data_ptr(), 0, st) == 0
    cache2 = torch.full((L.vad_ae_frame_cache_floats(2 * N),), 7.0, device=dev)
    outs = [torch.full((2 * N * k,), 7.0, device=dev) for k in (64, 1, 1, 1, 4096)]

    def call(nframes, T_, stride, w0, nw, c=cache):
        return L.vad_ae_windows_forward(pl.h, c.data_ptr(), frames.data_ptr(), nframes, T_, stride, w0, nw,
                                        *[o.data_ptr() for o in outs], st)

    for args, text in [((N, N + 1, 1, 0, 1), b"T must be in 1..nframes"),
                       ((N, 0, 1, 0, 1), b"T must be in 1..nframes"),
                       ((N, T, 0, 0, 1), b"stride must be >= 1"),
                       ((N, T, 1, 2, 2), b"w0 .. w0 + nw - 1 reach outside the video"),
                       ((N, T, 1, -1, 1), b"w0 .. w0 + nw - 1 reach outside the video"),
                       ((N, T, 2, 2, 1), b"w0 .. w0 + nw - 1 reach outside the video"),
                       ((2 * N, 1, 1, 0, N + 1, cache2), b"nw must be in 1..B"),
                       ((N, T, 1, 0, 0), b"nw must be in 1..B")]:
        assert call(*args) != 0, args
        assert text in L.vad_last_error(), L.vad_last_error()
    assert L.vad_ae_frames_forward(pl.h, frames.data_ptr(), 2 * N, cache2.data_ptr(), N + 1, st) != 0
    assert b"f0 .. f0 + F - 1" in L.vad_last_error(), L.vad_last_error()
    assert L.vad_ae_frames_forward(pl.h, frames.data_ptr(), N, cache2.data_ptr(), 1, st) != 0
    assert b"f0 .. f0 + F - 1" in L.vad_last_error(), L.vad_last_error()
    torch.cuda.synchronize()
    for o in outs + [cache2]:
        assert bool((o == 7.0).all())
    assert call(N, T, 1, 0, 3) == 0  # and the same call with legal arguments runs
    torch.cuda.synchronize()
    for o, k, width in zip(outs, ("sequence_features", "recon_errors", "memory_scores", "anomaly_scores",
                                  "reconstructed"), (64, 1, 1, 1, 4096)):
        assert torch.equal(o[:3 * width], ref[k].reshape(-1)), k
        assert bool((o[3 * width:] == 7.0).all()), k
