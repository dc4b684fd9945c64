"""CausalAnomalyDetector.open_stream_group on the GPU.  Stream s of a group must return what a CadStream on the same
frames returns, so every stream is held to the CPU oracle on its own stacked windows (oracle.cad_oracle.cad_forward at
clip index clip0[s] + w) at the project's forward tolerance rtol 1e-4 / atol 1e-5 with equal box counts and Nmax; a
group of one stream whose pushes are powers of two runs CadStream's frame and window counts and must equal it bit for
bit.  The table-addressed plan entries are also driven directly: what they store, where, and that a table the library
rejects launches nothing.  Helpers: those of tests/test_stream_gpu.py."""
import numpy as np
import pytest
import torch

from oracle import cad_oracle as co
from tests.golden.cases import FORCED_A
from tests.golden_util import make_cad_model
from tests.test_stream_gpu import (EMPTY_SHAPES, FORCED_SEED, THRESHOLDS, TOL, _assert_same_bits,
                                   _check_against_oracle, _concat, _oracle_windows)

pytestmark = pytest.mark.gpu

H = W = 64
T = 4
FIELDS = ("feats", "gi", "boxes", "counts", "slot")
SENTINEL = 0x7F4A11CE  # (a float32 bit pattern no kernel here produces; compared as int32)


def _push_group(g, frames, sizes):
    """Pushes sizes[p][s] frames of stream s at push p; returns the per-stream lists of per-push outputs."""
    S = len(frames)
    at, outs = [0] * S, [[] for _ in range(S)]
    for ks in sizes:
        res = g.push([frames[s][at[s]:at[s] + k] if k else None for s, k in enumerate(ks)])
        assert len(res) == S
        for s, k in enumerate(ks):
            at[s] += k
            assert g.frames_seen[s] == at[s]
            assert len(res[s]["detections"]) == k
            outs[s].append(res[s])
    assert at == [f.shape[0] for f in frames]
    return outs


def _assert_empty(p):
    for k, shape in EMPTY_SHAPES.items():
        assert p[k].shape == shape and p[k].is_cuda and p[k].dtype == torch.float32, k
    assert p["causal_factors"] == [] and p["window_starts"].shape == (0,) and p["window_starts"].dtype == torch.int64


def test_three_streams_in_lock_step():
    """Three streams of different content, clip0 = (3, 50, 1000), one frame each per push at max_push = 1 (cap = 4):
    twelve pushes wrap every ring three times.  A wrong base, slot or key gives another stream's numbers or noise."""
    case = dict(name="sg_lock", seed=0, forced=None)
    N, clip0 = 12, (3, 50, 1000)
    frames = [co.synth_clips(s, 0, 0, 1, N, H, W)[0] for s in (0, 1, 2)]
    m = make_cad_model(case).cuda().eval()
    g = m.open_stream_group(3, window=T, stride=1, max_push=1, seed=7, clip0=clip0)
    assert g.cap == 4 and g.total_slots == 12
    outs = _push_group(g, [f.cuda() for f in frames], [(1, 1, 1)] * N)
    assert g.windows_emitted == [9, 9, 9]
    for s in range(3):
        for p in outs[s][:3]:
            _assert_empty(p)
        for i, p in enumerate(outs[s][3:]):
            assert p["window_starts"].tolist() == [i] and p["anomaly_scores"].shape == (1,)
        ref = _oracle_windows(case, frames[s], T, 1, 7, 0, clip0[s])
        assert _check_against_oracle(_concat(outs[s]), ref, N, T, 1) == [1] * 9


RAGGED = [(3, 0, 1), (1, 2, 0), (0, 3, 3), (3, 2, 1), (2, 3, 0), (1, 0, 3), (0, 2, 1)]


@pytest.mark.parametrize("forced", [None, FORCED_A], ids=["fallback", "forced"])
def test_ragged_pushes(forced):
    """max_push = 3, stride 2, cap = 6, three streams of 10, 12 and 9 frames in pushes of 4, 3, 6, 6, 5, 4, 3 frames
    (plans of 4 and 8: padded and unpadded); in each stream one chunk straddles the wrap (frames 4-6, 5-6, 5-7).
    Reference init (fallback boxes) and forced detections with window-dependent Nmax.  Every stream against the
    oracle, and against a CadStream fed the same chunks, at the same tolerance."""
    case = dict(name="sg_ragged", seed=FORCED_SEED, forced=forced)
    stride, clip0 = 2, (5, 40, 900)
    lens = [sum(ks[s] for ks in RAGGED) for s in range(3)]
    assert lens == [10, 12, 9]
    frames = [co.synth_clips(cs, 0, 0, 1, n, H, W)[0] for cs, n in zip((134, 132, 137), lens)]
    refs = [_oracle_windows(case, frames[s], T, stride, 11, 2, clip0[s]) for s in range(3)]
    nmaxs = [[z.shape[0] for z in r["causal_factors"]] for r in refs]
    if forced:
        assert any(len(set(n)) >= 2 for n in nmaxs), f"fixture, not kernel: no stream's windows differ in Nmax {nmaxs}"
        for r in refs:
            boxes = r["boxes"].numpy()
            margin = min(float(np.abs(boxes[..., q] - t).min()) for q, ts in THRESHOLDS.items() for t in ts)
            assert margin >= 1e-3, f"fixture, not kernel: an oracle box lies {margin:.3g} px from a threshold"
    m = make_cad_model(case).cuda().eval()
    dev = [f.cuda() for f in frames]
    g = m.open_stream_group(3, window=T, stride=stride, max_push=3, seed=11, step=2, clip0=clip0)
    assert g.cap == 6
    outs = _push_group(g, dev, RAGGED)
    for s in range(3):
        out = _concat(outs[s])
        assert _check_against_oracle(out, refs[s], lens[s], T, stride) == nmaxs[s]
        single = m.open_stream(window=T, stride=stride, max_push=3, seed=11, step=2, clip0=clip0[s])
        f, want = 0, []
        for ks in RAGGED:
            if ks[s]:
                want.append(single.push(dev[s][f:f + ks[s]]))
                f += ks[s]
        want = _concat(want)
        assert out["window_starts"].tolist() == want["window_starts"].tolist()
        assert [z.shape for z in out["causal_factors"]] == [z.shape for z in want["causal_factors"]]
        assert [d.shape for d in out["detections"]] == [d.shape for d in want["detections"]]
        for k in ("anomaly_scores", "direct_predictions", "causal_anomaly_scores", "kl_losses", "adjacency_matrices"):
            np.testing.assert_allclose(out[k].cpu().numpy(), want[k].cpu().numpy(), err_msg=f"stream {s}: {k}", **TOL)
        for k in ("causal_factors", "detections"):
            for i, (a, b) in enumerate(zip(out[k], want[k])):
                np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), err_msg=f"stream {s}: {k}[{i}]", **TOL)


def test_stride_larger_than_the_window():
    """T = 2, stride 5 on two streams of 12 frames (cap = 4): windows at 0, 5, 10; the second push completes none in
    either stream (no window stage runs), the fourth and fifth none in one; frames 2-4 and 7-9 fill no window and
    still get detections, checked against the oracle's single-frame clips."""
    case = dict(name="sg_gaps", seed=0, forced=None)
    Tw, stride, N, clip0 = 2, 5, 12, (2, 70)
    frames = [co.synth_clips(cs, 0, 0, 1, N, H, W)[0] for cs in (4, 6)]
    m = make_cad_model(case).cuda().eval()
    g = m.open_stream_group(2, window=Tw, stride=stride, max_push=3, seed=3, step=1, clip0=clip0)
    assert g.cap == 4
    outs = _push_group(g, [f.cuda() for f in frames], [(3, 2), (3, 3), (3, 3), (3, 3), (0, 1)])
    assert [p["window_starts"].tolist() for p in outs[0]] == [[0], [], [5], [10], []]
    assert [p["window_starts"].tolist() for p in outs[1]] == [[0], [], [5], [], [10]]
    for s in range(2):
        for p in outs[s]:
            if p["window_starts"].numel() == 0:
                _assert_empty(p)
        out = _concat(outs[s])
        _check_against_oracle(out, _oracle_windows(case, frames[s], Tw, stride, 3, 1, clip0[s]), N, Tw, stride)
        single = _oracle_windows(case, frames[s], 1, 1, 0, 0, 0)
        for f in (2, 3, 4, 7, 8, 9):
            np.testing.assert_allclose(out["detections"][f].cpu().numpy(), single["detections"][f][0].numpy(),
                                       err_msg=f"stream {s}: boxes of frame {f}", **TOL)


def test_one_stream_is_cad_stream_bit_for_bit():
    """num_streams = 1, max_push = 4, pushes of 4, 4, 2, 1, 4: each runs the frame count and the window count of the
    same CadStream push, through the same arithmetic, so every key is bit-identical.  (A push of 3 pads to 4 frames
    and may pick another split-K: left out on purpose.)"""
    case = dict(name="sg_bits", seed=1, forced=FORCED_A)
    sizes = [4, 4, 2, 1, 4]
    frames = co.synth_clips(1, 0, 0, 1, sum(sizes), H, W)[0].cuda()
    m = make_cad_model(case).cuda().eval()
    s = m.open_stream(window=T, stride=1, max_push=4, seed=9, step=1, clip0=2)
    g = m.open_stream_group(1, window=T, stride=1, max_push=4, seed=9, step=1, clip0=2)
    f = 0
    for k in sizes:
        want = s.push(frames[f:f + k])
        got = g.push([frames[f:f + k]])
        assert len(got) == 1
        _assert_same_bits(got[0], want)
        f += k
    assert g.frames_seen == [s.frames_seen] and g.windows_emitted == [s.windows_emitted] == [12]


def _bound_plan(m, K):
    """The (K, 1, H, W) plan of m, built, bound and with fresh weight images (two pushes of a stream)."""
    frames = co.synth_clips(0, 0, 0, 1, 2 * K, H, W)[0].cuda()
    s = m.open_stream(window=T, max_push=K)
    s.push(frames[:K])
    s.push(frames[K:])
    return m.engine().plan(K, 1, H, W), frames


def _sentinel_cache(L, slots, dev):
    n = L.vad_cad_frame_cache_floats(slots)
    return torch.full((n,), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)


def test_group_store_writes_the_named_slots_and_nothing_else():
    """vad_cad_frames_forward_group on a cache of two rings of 5 slots prefilled with a sentinel, dst = (7, -1, 2, -1):
    slots 7 and 2 hold, bit for bit and in all five arrays, what vad_cad_frames_forward_ring stores for frames 0 and 2
    on the same plan; every other word of the cache is still the sentinel."""
    from vad_amd import _native as nat
    from vad_amd.video import cache_field
    L = nat.lib()
    m = make_cad_model(dict(name="sg_store", seed=0, forced=FORCED_A)).cuda().eval()
    K, slots = 4, 10
    pl, frames = _bound_plan(m, K)
    dev, st = frames.device, nat.stream_of(frames.device)
    x = frames[:K].contiguous()
    cache = _sentinel_cache(L, slots, dev)
    table = torch.zeros(L.vad_cad_group_table_bytes(K, K) // 4, dtype=torch.int32, device=dev)
    dst = torch.tensor([7, -1, 2, -1], dtype=torch.int32)
    nat.check(L.vad_cad_frames_forward_group(pl.h, x.data_ptr(), slots, cache.data_ptr(), dst.data_ptr(),
                                             table.data_ptr(), st))
    ring = _sentinel_cache(L, K, dev)
    nat.check(L.vad_cad_frames_forward_ring(pl.h, x.data_ptr(), K, ring.data_ptr(), 0, st))
    torch.cuda.synchronize()
    for name in FIELDS:
        got = cache_field(cache, slots, name).view(torch.int32)
        want = cache_field(ring, K, name).view(torch.int32)
        for slot, f in ((7, 0), (2, 2)):
            assert bool((want[f] != SENTINEL).all()), f"fixture, not kernel: the ring store left {name} of frame {f}"
            assert torch.equal(got[slot], want[f]), f"{name} of slot {slot}"
    # every word outside the two named slots of the five arrays: blank the named rows, then the cache is all sentinel
    rest = cache.clone()
    for name in FIELDS:
        v = cache_field(rest, slots, name).view(torch.int32)
        v[7] = SENTINEL
        v[2] = SENTINEL
    assert bool((rest.view(torch.int32) == SENTINEL).all())


def test_group_abi_errors_launch_nothing():
    """A duplicate dst, dst = total_slots, a base that is no multiple of cap, base + cap > total_slots, first = cap,
    nw = B + 1, T = cap + 1 and null tables: non-zero, a message that names the entry or the argument, and the sentinel
    cache and outputs untouched.  The same calls with legal tables run."""
    from vad_amd import _native as nat
    L = nat.lib()
    m = make_cad_model(dict(name="sg_abi", seed=0, forced=None)).cuda().eval()
    K, cap, slots = 4, 5, 10
    pl, frames = _bound_plan(m, K)
    dev, st = frames.device, nat.stream_of(frames.device)
    x = frames[:K].contiguous()
    cache = _sentinel_cache(L, slots, dev)
    table = torch.zeros(L.vad_cad_group_table_bytes(K, K) // 4, dtype=torch.int32, device=dev)
    n = 8
    outs = [torch.full((n * k,), 7.0, device=dev) for k in (1, 2, 1, 1, 30, 36)]
    nmax = torch.full((n,), 7, dtype=torch.int32, device=dev)

    host = []  # (the host tables stay alive until the device is idle)

    def store(dst, dev_table=True):
        if dst is not None:
            host.append(torch.tensor(dst, dtype=torch.int32))
        return L.vad_cad_frames_forward_group(pl.h, x.data_ptr(), slots, cache.data_ptr(),
                                              None if dst is None else host[-1].data_ptr(),
                                              table.data_ptr() if dev_table else None, st)

    def score(rows, Tw=T, host_table=True):
        host.append(torch.tensor(rows, dtype=torch.int64))
        return L.vad_cad_windows_forward_group(pl.h, cache.data_ptr(), slots, cap, Tw,
                                               host[-1].data_ptr() if host_table else None, len(rows),
                                               table.data_ptr(), 0, 0, *[o.data_ptr() for o in outs], nmax.data_ptr(),
                                               st)

    ok = (0, 0, 0)
    for call, text in [
            (lambda: store([0, 3, 3, -1]), b"two entries of dst name slot 3"),
            (lambda: store([0, 1, slots, -1]), b"dst[2] = 10 is outside"),
            (lambda: store([0, -2, 1, 2]), b"dst[1] = -2 is outside"),
            (lambda: store(None), b"null table"),
            (lambda: store([0, 1, 2, 3], dev_table=False), b"null table"),
            (lambda: score([ok, (3, 0, 0)]), b"window 1 (base 3, first 0): base must be a non-negative multiple"),
            (lambda: score([(10, 0, 0)]), b"window 0 (base 10, first 0): base + cap exceeds total_slots"),
            (lambda: score([ok, ok, (5, cap, 0)]), b"window 2 (base 5, first 5): first must be in 0..cap - 1"),
            (lambda: score([ok] * (K + 1)), b"nw must be in 1..the plan's B"),
            (lambda: score([ok], Tw=cap + 1), b"T must be in 1..cap"),
            (lambda: score([ok], host_table=False), b"null table")]:
        assert call() != 0
        assert text in L.vad_last_error(), L.vad_last_error()
    torch.cuda.synchronize()
    assert bool((cache.view(torch.int32) == SENTINEL).all())
    for o in outs:
        assert bool((o == 7.0).all())
    assert bool((nmax == 7).all())
    # and the same calls with legal tables run: four frames into ring 1, one window over them
    assert store([5, 6, 7, 8]) == 0
    assert score([(5, 0, 0)]) == 0
    torch.cuda.synchronize()
    assert bool((nmax[:1] == 1).all()) and bool((nmax[1:] == 7).all())
    assert bool((outs[0][1:] == 7.0).all()) and 0.0 <= float(outs[0][0]) <= 1.0


def test_isolation_from_other_work_on_the_same_plans():
    """Between the pushes of a two-stream group: a clip forward on the group's own (4, 1, H, W) plan shape, a
    score_video call and a CadStream push.  The group's outputs equal an undisturbed group's bit for bit, and pushing
    changes no parameter or buffer."""
    case = dict(name="sg_iso", seed=2, forced=FORCED_A)
    m = make_cad_model(case).cuda().eval()
    frames = [co.synth_clips(cs, 0, 0, 1, 8, H, W)[0].cuda() for cs in (3, 8)]
    other = co.synth_clips(5, 0, 0, 4, 1, H, W).cuda()
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    sizes = [(2, 2), (2, 1), (2, 2), (2, 3)]

    def run(disturb):
        g = m.open_stream_group(2, window=T, max_push=3, seed=6, clip0=(0, 100))
        side = m.open_stream(window=T, max_push=4)
        at, outs = [0, 0], [[], []]
        for ks in sizes:
            res = g.push([frames[s][at[s]:at[s] + k] for s, k in enumerate(ks)])
            for s, k in enumerate(ks):
                at[s] += k
                outs[s].append(res[s])
            if disturb:
                with torch.no_grad():
                    m(other, seed=4)
                m.score_video(frames[0][2:], window=T, stride=1, chunk=4)
                side.push(frames[1][:4])
        return [_concat(o) for o in outs]

    quiet, loud = run(False), run(True)
    for s in range(2):
        assert quiet[s]["anomaly_scores"].shape == (5,)
        _assert_same_bits(loud[s], quiet[s])
    for k, v in m.state_dict().items():
        assert torch.equal(v, state[k]), f"{k} changed"
