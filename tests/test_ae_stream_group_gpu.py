"""VideoAutoEncoder.open_stream_group on the GPU.  Stream s of a group must return what an AeStream on the same frames
returns, so every stream is held to the CPU oracle on its own stacked windows (oracle.ae_oracle.ae_eval_batch) at the
tolerances of tests/test_ae_score_video_gpu.py, whose helpers these are; a group of one stream whose pushes are powers
of two runs AeStream's frame and window counts and must equal it bit for bit.  The table-addressed plan entries are
also driven directly: what they store, where, and that arguments the library rejects launch nothing.

Two fixture conditions, asserted from the oracle alone in every case, so that a slot mix-up cannot pass: (a) adjacent
oracle windows of a stream differ in every compared output by at least 10x its tolerance (assert_windows_differ), and
(b) any two windows of two different streams differ in sequence_features by at least 10x its tolerance
(assert_streams_differ).  The (model seed, frame seed) pairs were chosen on the oracle alone."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import ae_oracle as ae
from tests.test_ae_score_video_gpu import (ALL, TOL, TOL_ERR, assert_windows_differ, check_against_oracle, make_frames,
                                           make_model, oracle_windows)
from tests.test_ae_stream_gpu import EMPTY_SHAPES, KEYS, _assert_same_bits, _concat

pytestmark = pytest.mark.gpu

HW = 64
WIDTHS = (("lat", 64), ("gx", 256), ("pix", 4096))
SENTINEL = 0x7F4A11CE  # (a float32 bit pattern no kernel here produces; compared as int32)


def assert_streams_differ(refs):
    """Condition (b): every window of one stream against every window of another, in the oracle's sequence features."""
    feats = [r["outputs"]["sequence_feature"].double() for r in refs]
    for i in range(len(feats)):
        for j in range(i + 1, len(feats)):
            a, b = feats[i][:, None, :], feats[j][None, :, :]
            d = (a - b).abs().amax(-1)
            need = 10 * (TOL["atol"] + TOL["rtol"] * torch.maximum(a.abs().amax(-1), b.abs().amax(-1)))
            worst = float((d / need).min())
            assert worst >= 1, (f"fixture, not kernel: a window of stream {i} and one of stream {j} differ by only "
                                f"{10 * worst:.3g}x the tolerance")


def _case(model_seed, frame_seeds, lens, T, stride):
    """One model, one video per stream and the oracle's windows of each; both fixture conditions asserted."""
    m = make_model(model_seed)
    frames = [make_frames(fs, n) for fs, n in zip(frame_seeds, lens)]
    refs = [oracle_windows(m, f, T, stride) for f in frames]
    for r in refs:
        assert_windows_differ(r, ALL)
    assert_streams_differ(refs)
    return m, frames, refs


@pytest.fixture(scope="module")
def lock_case():
    """Model 46, T = 4, stride 1, three streams of 11 frames: computed once, shared by the tests that only read it."""
    return _case(46, (1, 2, 3), (11, 11, 11), 4, 1)


def _push_group(g, frames, sizes):
    """Pushes sizes[p][s] frames of stream s at push p -- where that is 0, None at even p and an empty (0, 1, 64, 64)
    tensor at odd p; returns the per-stream lists of per-push outputs.  No device value is read here."""
    S = len(frames)
    at, outs = [0] * S, [[] for _ in range(S)]
    for p, ks in enumerate(sizes):
        res = g.push([frames[s][at[s]:at[s] + k] if k or p % 2 else None for s, k in enumerate(ks)])
        assert isinstance(res, list) and len(res) == S
        for s, k in enumerate(ks):
            at[s] += k
            assert g.frames_seen[s] == at[s]
            assert res[s]["frame_features"].shape == (k, 64) and res[s]["frame_features"].is_cuda
            outs[s].append(res[s])
    assert at == [f.shape[0] for f in frames]
    return outs


def _assert_empty(p, recon=True):
    for k, shape in EMPTY_SHAPES.items():
        if k == "reconstructed" and not recon:
            continue
        assert p[k].shape == shape and p[k].is_cuda and p[k].dtype == torch.float32, k
    assert p["window_starts"].shape == (0,) and p["window_starts"].dtype == torch.int64
    assert p["window_starts"].device.type == "cpu"


def test_three_streams_in_lock_step_on_the_smallest_ring(lock_case):
    """max_push = 1, cap = T = 4: eleven pushes of one frame per stream (F = 3: the plan size is the cap, not 4); the
    first three return empty dicts, every later window but the first reads across the wrap of its ring.  A wrong base
    or slot gives another stream's numbers."""
    m, frames, refs = lock_case
    N, T = 11, 4
    g = m.cuda().open_stream_group(3, window=T, stride=1, max_push=1, return_reconstructions=True)
    assert (g.cap, g.total_slots, g.max_frames) == (4, 12, 3)
    outs = _push_group(g, [f.cuda() for f in frames], [(1, 1, 1)] * N)
    assert g.windows_emitted == [8, 8, 8] and g.frames_seen == [N] * 3
    for s in range(3):
        for p in outs[s][:3]:
            _assert_empty(p)
            assert set(p) == set(KEYS) | {"window_starts"}
        for i, p in enumerate(outs[s][3:]):
            assert p["window_starts"].tolist() == [i] and p["anomaly_scores"].shape == (1,)
            assert p["window_starts"].dtype == torch.int64 and p["window_starts"].device.type == "cpu"
        check_against_oracle(_concat(outs[s]), refs[s], N, T, 1, ALL)


RAGGED = [(3, 2, 0), (1, 3, 3), (2, 0, 0), (3, 3, 3), (3, 3, 1), (0, 3, 0), (2, 3, 2), (3, 3, 3), (3, 0, 0)]


def test_ragged_pushes_with_the_wrap_at_every_step_of_the_prefetch():
    """T = 7, max_push = 3, cap = 9, streams of 20, 20 and 12 frames, each on its own push pattern with k_s in 0..3:
    None entries, empty tensors, pushes where one stream alone brings frames (the third and the sixth), plans of 2, 4,
    8 and 9 frames (padded, unpadded and the cap).  The streams' windows together start in every slot 0..8, so the
    wrap falls at every t of a window -- inside a prefetch group and at the t + AE_PF look-ahead."""
    T, cap, lens = 7, 9, (20, 20, 12)
    assert [sum(ks[s] for ks in RAGGED) for s in range(3)] == list(lens)
    assert sorted({sum(ks) for ks in RAGGED}) == [2, 3, 5, 7, 9] and [ks for ks in RAGGED if sum(ks) == max(ks)]
    m, frames, refs = _case(55, (24, 37, 3), lens, T, 1)
    g = m.cuda().open_stream_group(3, window=T, stride=1, max_push=3, return_reconstructions=True)
    assert g.cap == cap and g.max_frames == 9
    outs = _push_group(g, [f.cuda() for f in frames], RAGGED)
    slots = set()
    for s in range(3):
        out = _concat(outs[s])
        starts = out["window_starts"].tolist()
        assert starts == list(range(lens[s] - T + 1))
        slots |= {w % cap for w in starts}
        for p in outs[s]:
            if p["window_starts"].numel() == 0:
                _assert_empty(p)
        check_against_oracle(out, refs[s], lens[s], T, 1, ALL)
    assert sorted(slots) == list(range(cap))
    assert g.windows_emitted == [14, 14, 6]


def test_stride_two_and_several_windows_per_stream_per_push():
    """T = 5, stride 2, max_push = 4, cap = 8, two streams of 13 frames in pushes of (4, 3), (4, 4), (4, 2), (1, 4):
    stream 0 completes 0, 2, 2, 1 windows, stream 1 completes 0, 2, 1, 2."""
    N, T, stride = 13, 5, 2
    m, frames, refs = _case(54, (15, 18), (N, N), T, stride)
    g = m.cuda().open_stream_group(2, window=T, stride=stride, max_push=4, return_reconstructions=True)
    assert g.cap == 8
    outs = _push_group(g, [f.cuda() for f in frames], [(4, 3), (4, 4), (4, 2), (1, 4)])
    assert [p["window_starts"].tolist() for p in outs[0]] == [[], [0, 2], [4, 6], [8]]
    assert [p["window_starts"].tolist() for p in outs[1]] == [[], [0, 2], [4], [6, 8]]
    for s in range(2):
        check_against_oracle(_concat(outs[s]), refs[s], N, T, stride, ALL)


def test_frames_that_belong_to_no_window():
    """T = 2, stride 5, max_push = 3, cap = 4 on the same two videos, cut to 13 and 11 frames: windows at 0 and 5 (and
    10 in stream 0); frames 2-4, 7-9 and 12 (10 in stream 1) fill no window and still return frame_features, checked
    against the oracle's encoder; the second and the fourth push complete no window in either stream, so no window
    stage runs."""
    T, stride, lens = 2, 5, (13, 11)
    m, frames, refs = _case(54, (15, 18), lens, T, stride)
    g = m.cuda().open_stream_group(2, window=T, stride=stride, max_push=3)
    assert g.cap == 4
    outs = _push_group(g, [f.cuda() for f in frames], [(3, 2), (2, 2), (3, 3), (3, 3), (2, 1)])
    assert [p["window_starts"].tolist() for p in outs[0]] == [[0], [], [5], [], [10]]
    assert [p["window_starts"].tolist() for p in outs[1]] == [[0], [], [5], [], []]
    params, bufs, _ = refs[0]["state"]
    for s, gaps in enumerate(([2, 3, 4, 7, 8, 9, 12], [2, 3, 4, 7, 8, 9, 10])):
        for p in outs[s]:
            assert "reconstructed" not in p
            if p["window_starts"].numel() == 0:
                _assert_empty(p, recon=False)
        out = _concat(outs[s])
        check_against_oracle(out, refs[s], lens[s], T, stride, ALL)
        with torch.no_grad():
            lat = ae.nan0(ae.encoder(params, bufs, frames[s][gaps], False))
        for a, b in zip(lat[:-1], lat[1:]):
            assert float((a - b).abs().max()) >= 10 * (1e-5 + 1e-4 * float(lat.abs().max())), \
                "fixture, not kernel: the oracle's latents of two gap frames are too close to tell apart"
        np.testing.assert_allclose(out["frame_features"][gaps].cpu().numpy(), lat.numpy(), **TOL)


def _with_nan_runs(frames):
    frames = frames.clone()
    frames[2, 0, 5, 7:40] = float("nan")
    frames[6, 0, 60, :] = float("nan")
    frames[9, 0, :, 3] = float("nan")
    return frames


@pytest.mark.parametrize("nan", [False, True], ids=["clean", "nan"])
def test_one_stream_is_ae_stream_bit_for_bit(nan):
    """num_streams = 1, max_push = 4, pushes of 4, 4, 2, 1, 4 frames: each runs the frame count (a power of two: no
    padding) and the window count of the same AeStream push, through the same arithmetic, so every key is
    bit-identical -- on clean frames and on frames with runs of NaN pixels."""
    T, sizes = 4, [4, 4, 2, 1, 4]
    m = make_model(50).cuda()
    frames = make_frames(11, sum(sizes))
    if nan:
        frames = _with_nan_runs(frames)
    frames = frames.cuda()
    s = m.open_stream(window=T, stride=1, max_push=4, return_reconstructions=True)
    g = m.open_stream_group(1, window=T, stride=1, max_push=4, return_reconstructions=True)
    f, worst = 0, 0.0
    for k in sizes:
        want = s.push(frames[f:f + k])
        got = g.push([frames[f:f + k]])
        assert len(got) == 1
        for key in KEYS:
            assert bool(torch.isfinite(got[0][key]).all()), key
            if want[key].numel():
                worst = max(worst, float((got[0][key] - want[key]).abs().max()))
        _assert_same_bits(got[0], want)
        assert got[0]["window_starts"].dtype == want["window_starts"].dtype
        f += k
    print(f"ae stream group vs ae stream ({'nan' if nan else 'clean'}): max abs diff {worst:.3g}")
    assert g.frames_seen == [s.frames_seen] and g.windows_emitted == [s.windows_emitted] == [12]


def test_nan_pixels_in_one_stream_leave_the_others_alone(lock_case):
    """Stream 1 with runs of NaN pixels: streams 0 and 2 return, bit for bit, what they return beside a clean stream
    1; stream 1 itself returns what it returns for the same frames with the NaN pixels set to 0."""
    m, frames, _ = lock_case
    md = m.cuda()
    sizes = [(2, 2, 2)] * 5 + [(1, 1, 1)]
    dirty = _with_nan_runs(frames[1])
    assert int(torch.isnan(dirty).sum()) > 100

    def run(middle):
        g = md.open_stream_group(3, window=4, max_push=2, return_reconstructions=True)
        return [_concat(o) for o in _push_group(g, [frames[0].cuda(), middle.cuda(), frames[2].cuda()], sizes)]

    clean, nan, zeroed = run(frames[1]), run(dirty), run(torch.nan_to_num(dirty, nan=0.0))
    for s in (0, 2):
        _assert_same_bits(nan[s], clean[s])
    _assert_same_bits(nan[1], zeroed[1])
    for k in KEYS:
        assert bool(torch.isfinite(nan[1][k]).all()), k
    assert not torch.equal(nan[1]["anomaly_scores"], clean[1]["anomaly_scores"])


def _bound_plan(m, K):
    """The (K, 1) plan of m, built and bound (one push of a stream), and 2K frames."""
    frames = make_frames(17, 2 * K).cuda()
    m.open_stream(window=4, max_push=K).push(frames[:K])
    return m.engine().plan(K, 1), frames


def _sentinel(n, dev, dtype=torch.float32):
    return torch.full((n,), SENTINEL, dtype=torch.int32, device=dev).view(dtype)


def _field(L, ring, slots, name):
    i, width = [(i, w) for i, (n, w) in enumerate(WIDTHS) if n == name][0]
    off = L.vad_ae_ring_offset(slots, i)
    return ring[off:off + slots * width].view(slots, width)


def test_group_store_writes_the_named_slots_and_nothing_else():
    """vad_ae_frames_forward_group on two rings of 5 slots and a device table, both prefilled with a sentinel, dst =
    (7, -1, 2, 9) -- a padding frame and the last slot of the last ring: slots 7, 2 and 9 hold, bit for bit and in all
    three arrays, what vad_ae_frames_forward_ring stores for frames 0, 2 and 3 on the same plan; every other word of
    the ring is still the sentinel, and the table holds the four destinations and nothing else."""
    from vad_amd import _native as nat
    L = nat.lib()
    m = make_model(53).cuda()
    K, slots = 4, 10
    pl, frames = _bound_plan(m, K)
    dev, st = frames.device, nat.stream_of(frames.device)
    x = frames[:K].contiguous()
    nb = L.vad_ae_group_table_bytes(K, K)
    assert nb == 16 + K * 16 and L.vad_ae_group_table_bytes(5, 2) == 32 + 32
    assert L.vad_ae_group_table_bytes(0, 1) == -1 and L.vad_ae_group_table_bytes(1, -1) == -1
    assert b"vad_ae_group_table_bytes" in L.vad_last_error()
    ring = _sentinel(L.vad_ae_ring_floats(slots), dev)
    table = _sentinel(nb // 4, dev, torch.int32)
    dst = torch.tensor([7, -1, 2, 9], dtype=torch.int32)
    nat.check(L.vad_ae_frames_forward_group(pl.h, x.data_ptr(), slots, ring.data_ptr(), dst.data_ptr(),
                                            table.data_ptr(), st))
    one = _sentinel(L.vad_ae_ring_floats(K), dev)
    nat.check(L.vad_ae_frames_forward_ring(pl.h, x.data_ptr(), K, one.data_ptr(), 0, st))
    torch.cuda.synchronize()
    assert table[:K].tolist() == dst.tolist() and bool((table[K:] == SENTINEL).all())
    for name, _ in WIDTHS:
        got = _field(L, ring, slots, name).view(torch.int32)
        want = _field(L, one, K, name).view(torch.int32)
        for slot, f in ((7, 0), (2, 2), (9, 3)):
            assert bool((want[f] != SENTINEL).all()), f"fixture, not kernel: the ring store left {name} of frame {f}"
            assert torch.equal(got[slot], want[f]), f"{name} of slot {slot}"
    assert torch.equal(_field(L, ring, slots, "pix")[9], x[3].view(-1))
    # every word outside the three named slots of the three arrays: blank the named rows, then all is sentinel
    rest = ring.clone()
    for name, _ in WIDTHS:
        _field(L, rest, slots, name).view(torch.int32)[[7, 2, 9]] = SENTINEL
    assert bool((rest.view(torch.int32) == SENTINEL).all())


def test_group_abi_errors_launch_nothing():
    """Every argument and table entry the library rejects: non-zero, a message that names it, and the sentinel ring,
    table and outputs untouched.  The same calls with legal tables then run and give an AeStream's results."""
    from vad_amd import _native as nat
    L = nat.lib()
    K, T, cap, slots = 4, 4, 5, 10
    m = make_model(53).cuda()
    pl, frames = _bound_plan(m, K)
    want = m.open_stream(window=T, max_push=K, return_reconstructions=True).push(frames[:K])
    assert want["window_starts"].tolist() == [0]
    pl_t3 = m.engine().plan(K, 3)
    unbound = ctypes.c_void_p()
    assert L.vad_ae_create(K, 1, ctypes.byref(unbound)) == 0
    dev, st = frames.device, nat.stream_of(frames.device)
    x = frames[:K].contiguous()
    ring = _sentinel(L.vad_ae_ring_floats(slots), dev)
    table = _sentinel(L.vad_ae_group_table_bytes(K, K) // 4, dev, torch.int32)
    n = 2 * K
    outs = [torch.full((n * w,), 7.0, device=dev) for w in (64, 1, 1, 1, 4096)]
    po = [o.data_ptr() for o in outs]
    xp, rp, tp = x.data_ptr(), ring.data_ptr(), table.data_ptr()
    host = []  # (the host tables stay alive until the device is idle)
    good_dst, ok = [5, 6, 7, 8], (5, 0)

    def store(dst=good_dst, plan=pl.h, x_=xp, slots_=slots, ring_=rp, table_=tp):
        if dst is not None:
            host.append(torch.tensor(dst, dtype=torch.int32))
        return L.vad_ae_frames_forward_group(plan, x_, slots_, ring_, None if dst is None else host[-1].data_ptr(),
                                             table_, st)

    def score(rows=(ok,), plan=pl.h, ring_=rp, slots_=slots, cap_=cap, T_=T, nw=None, table_=tp, ptrs=po):
        if rows is not None:
            host.append(torch.tensor(rows, dtype=torch.int64))
        return L.vad_ae_windows_forward_group(plan, ring_, slots_, cap_, T_,
                                              None if rows is None else host[-1].data_ptr(),
                                              len(rows) if nw is None else nw, table_, *ptrs, st)

    try:
        for call, text in [
                (lambda: store(plan=None), b"null plan"),
                (lambda: store(plan=unbound), b"plan not bound"),
                (lambda: store(plan=pl_t3.h), b"T = 1"),
                (lambda: store(x_=None), b"frames_chunk must be a 16-byte aligned device pointer"),
                (lambda: store(x_=xp + 4), b"frames_chunk must be a 16-byte aligned device pointer"),
                (lambda: store(ring_=None), b"ring must be a 16-byte aligned device pointer"),
                (lambda: store(ring_=rp + 4), b"ring must be a 16-byte aligned device pointer"),
                (lambda: store(dst=None), b"null table (host_dst)"),
                (lambda: store(table_=None), b"dev_table must be a 16-byte aligned device pointer"),
                (lambda: store(table_=tp + 4), b"dev_table must be a 16-byte aligned device pointer"),
                (lambda: store(slots_=0), b"total_slots must be in 1..2^24"),
                (lambda: store(slots_=(1 << 24) + 1), b"total_slots must be in 1..2^24"),
                (lambda: store([0, 3, 3, -1]), b"two entries of dst name slot 3"),
                (lambda: store([0, 1, slots, -1]), b"dst[2] = 10 is outside"),
                (lambda: store([0, -2, 1, 2]), b"dst[1] = -2 is outside")]:
            assert call() != 0
            assert b"vad_ae_frames_forward_group" in L.vad_last_error() and text in L.vad_last_error(), \
                L.vad_last_error()
        for call, text in [
                (lambda: score(plan=None), b"null plan"),
                (lambda: score(plan=unbound), b"plan not bound"),
                (lambda: score(plan=pl_t3.h), b"T = 1"),
                (lambda: score(ring_=None), b"ring must be a 16-byte aligned device pointer"),
                (lambda: score(ring_=rp + 4), b"ring must be a 16-byte aligned device pointer"),
                (lambda: score(rows=None, nw=1), b"null table (host_windows)"),
                (lambda: score(table_=None), b"dev_table must be a 16-byte aligned device pointer"),
                (lambda: score(table_=tp + 8), b"dev_table must be a 16-byte aligned device pointer"),
                (lambda: score(ptrs=[None] + po[1:]), b"seq (16-byte aligned)"),
                (lambda: score(ptrs=[po[0] + 4] + po[1:]), b"seq (16-byte aligned)"),
                (lambda: score(ptrs=po[:1] + [None] + po[2:]), b"must not be null"),
                (lambda: score(ptrs=po[:3] + [None] + po[4:]), b"must not be null"),
                (lambda: score(cap_=0), b"cap must be >= 1"),
                (lambda: score(slots_=0), b"total_slots must be in 1..2^24 and a multiple of cap"),
                (lambda: score(slots_=((1 << 24) // cap + 1) * cap), b"total_slots must be in 1..2^24"),
                (lambda: score(slots_=slots + 1), b"a multiple of cap"),
                (lambda: score(T_=0), b"T must be in 1..cap"),
                (lambda: score(T_=cap + 1), b"T must be in 1..cap"),
                (lambda: score(rows=((0, 0),), slots_=5000, cap_=5000, T_=4097), b"T must be at most 4096"),
                (lambda: score(nw=0), b"nw must be in 1..B"),
                (lambda: score([ok] * (K + 1)), b"nw must be in 1..B"),
                (lambda: score([ok, (3, 0)]), b"window 1 (base 3, first 0): base must be a non-negative multiple"),
                (lambda: score([(-5, 0)]), b"window 0 (base -5, first 0): base must be a non-negative multiple"),
                (lambda: score([(10, 0)]), b"window 0 (base 10, first 0): base + cap exceeds total_slots"),
                (lambda: score([ok, ok, (5, cap)]), b"window 2 (base 5, first 5): first must be in 0..cap - 1"),
                (lambda: score([(0, -1)]), b"window 0 (base 0, first -1): first must be in 0..cap - 1")]:
            assert call() != 0
            assert b"vad_ae_windows_forward_group" in L.vad_last_error() and text in L.vad_last_error(), \
                L.vad_last_error()
    finally:
        L.vad_ae_destroy(unbound)
    torch.cuda.synchronize()
    assert bool((ring.view(torch.int32) == SENTINEL).all()) and bool((table == SENTINEL).all())
    for o in outs:
        assert bool((o == 7.0).all())
    # and the same calls with legal tables run: four frames into ring 1, one window over them
    assert store() == 0 and score() == 0
    torch.cuda.synchronize()
    for o, k, width in zip(outs, ("sequence_features", "recon_errors", "memory_scores", "anomaly_scores",
                                  "reconstructed"), (64, 1, 1, 1, 4096)):
        assert torch.equal(o[:width], want[k].reshape(-1)), k
        assert bool((o[width:] == 7.0).all()), k
    assert torch.equal(_field(L, ring, slots, "lat")[5:9], want["frame_features"])
    assert bool((_field(L, ring, slots, "lat").view(torch.int32)[:5] == SENTINEL).all())


def test_back_to_back_pushes_keep_their_own_tables(lock_case):
    """max_push = 2 (cap = 5): after the rings are filled, two pushes with different tables -- (2, 1, 0) and
    (1, 2, 2) frames -- and no host read of a device value between them or before them; the outputs are read only
    after the second.  Both match the oracle: the second push's host tables were not written over the first's before
    the device had copied them."""
    m, frames, refs = lock_case
    T = 4
    dev = [f.cuda() for f in frames]
    g = m.cuda().open_stream_group(3, window=T, max_push=2)
    torch.cuda.synchronize()
    g.push([f[0:2] for f in dev])
    g.push([f[2:4] for f in dev])
    a = g.push([dev[0][4:6], dev[1][4:5], None])
    b = g.push([dev[0][6:7], dev[1][5:7], dev[2][4:6]])
    assert [p["window_starts"].tolist() for p in a] == [[1, 2], [1], []]
    assert [p["window_starts"].tolist() for p in b] == [[3], [2, 3], [1, 2]]
    torch.cuda.synchronize()
    for res in (a, b):
        for s, p in enumerate(res):
            ws = p["window_starts"].tolist()
            o = refs[s]["outputs"]
            for k, v, tol in (("sequence_features", o["sequence_feature"], TOL),
                              ("memory_scores", o["anomaly_score"], TOL),
                              ("recon_errors", refs[s]["recon_error"], TOL_ERR),
                              ("anomaly_scores", refs[s]["combined"], TOL)):
                np.testing.assert_allclose(p[k].cpu().numpy(), v[ws].numpy(), err_msg=f"stream {s}: {k}", **tol)


def test_isolation_from_other_work_on_the_same_plans():
    """Between the pushes of a two-stream group: a clip forward on the group's own (4, 1) plan shape, a score_video
    call, an AeTrainer.eval_batch and an AeStream push.  The group's outputs equal an undisturbed group's bit for bit,
    and pushing changes no parameter or buffer."""
    from vad_amd.ae import AeTrainer
    T = 4
    m = make_model(52).cuda()
    frames = [make_frames(fs, 9).cuda() for fs in (15, 16)]
    clips = ae.synth_clips(52, 0, 0, 2, T).cuda()
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    for name in ("running_mean", "running_var", "num_batches_tracked", "normal_memory", "memory_ptr"):
        assert any(k.endswith(name) for k in state), name
    sizes = [(2, 2), (2, 1), (2, 2), (2, 3), (1, 1)]

    def run(disturb):
        g = m.open_stream_group(2, window=T, max_push=3, return_reconstructions=True)
        side = m.open_stream(window=T, max_push=4)
        at, outs = [0, 0], [[], []]
        for ks in sizes:
            res = g.push([frames[s][at[s]:at[s] + k] for s, k in enumerate(ks)])
            for s, k in enumerate(ks):
                at[s] += k
                outs[s].append(res[s])
            if disturb:
                with torch.no_grad():
                    m(frames[1][2:6].view(4, 1, 1, HW, HW))
                    m(clips)
                m.score_video(frames[0][1:], window=T, stride=1, chunk=4)
                AeTrainer(m).eval_batch(clips)
                side.push(frames[1][:4])
        return [_concat(o) for o in outs]

    quiet, loud = run(False), run(True)
    for s in range(2):
        assert quiet[s]["anomaly_scores"].shape == (6,)
        _assert_same_bits(loud[s], quiet[s])
    for k, v in m.state_dict().items():
        assert torch.equal(v, state[k]), f"{k} changed"
