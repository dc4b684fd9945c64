"""ClipStreamGroup on the GPU, for the a2, minicausal (grey and 3-channel) and bbox clip models: one push takes frames
of several cameras, scatters them into the cameras' rings -- one allocation -- and scores the windows they complete with
one windows call whose first conv finds every window through a (base, first) row of a device table.

The criterion is test_clip_stream_gpu.py's: a windows call on nw windows runs the clip path's kernels on nw clips, so
the outputs of a push, concatenated in camera order, must equal ``model(clips)`` on those windows gathered with torch
into one batch in that order, bit for bit (a2, a single window: the clip twice, row 0).  And against one ClipStream per
camera fed the same frames: the batches differ there -- a lone stream runs 1 or 2 windows, the group up to 6 -- which
leaves minicausal equal bit for bit (no kernel is chosen by the batch), and bbox and a2 too as long as both sides stay
in the same kernels: bbox's head GEMMs up to 8 rows, a2's conv GEMMs up to 14 clips at 10 x 13 frames and T = 4 (the
derivation is test_clip_stream_gpu.py's docstring).  No push here completes more than 6 windows, so every comparison is
torch.equal.

window 4 and max_push 2 make rings of 5 slots, ring s in slots 5 s .. 5 s + 4.  The 14 pushes of PUSHES bring every
camera's frames in another rhythm -- None, an empty tensor, one frame, two; camera 2 starts when camera 0 has six
frames -- and start a push at every slot of every ring; windows straddle each ring's end with their first frame, in
their middle and before their last frame.  With stride 3 four of the pushes complete no window anywhere."""
import pytest
import torch

from tests.test_clip_score_video_gpu import CHANNELS, KEYS, KINDS, assert_same, clip_call, gather, make, video
from vad_amd import _native as nat
from vad_amd import data

pytestmark = pytest.mark.gpu

H, W, T, CAP = 10, 13, 4, 5
# per push: the number of frames of cameras 0, 1, 2 (None: the entry is None; 0: an empty tensor)
PUSHES = [(2, 1, None), (2, 2, None), (2, None, None), (2, 1, 1), (2, 2, 2), (1, 0, 2), (2, 1, 1), (None, 2, 1),
          (1, 2, 2), (2, None, 2), (2, 1, 1), (1, 2, 2), (None, 1, 1), (2, 2, 2)]
TOTAL = [sum(k or 0 for k in col) for col in zip(*PUSHES)]  # 21, 17, 17 frames


def entries(xs, seen, ks):
    """The list a push takes: camera s's next ks[s] frames of xs[s]."""
    return [None if k is None else xs[s][seen[s]:seen[s] + k] for s, k in enumerate(ks)]


def completed(seen, k, stride, window=T):
    """The starts of the windows that frames seen .. seen + k - 1 of a camera complete."""
    return [s for s in range(0, seen + k - window + 1, stride) if s + window > seen]


def empty(kind, o):
    return all(o[k].shape[0] == 0 and o[k].is_cuda for k in KEYS[kind]) and o["window_starts"].tolist() == []


def cat_cameras(kind, outs):
    return tuple(torch.cat([o[k] for o in outs]) for k in KEYS[kind])


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_three_cameras_out_of_step(kind, stride):
    m = make(kind)
    C = CHANNELS[kind]
    xs = [video(60 + 10 * s + stride, TOTAL[s], C, H, W) for s in range(3)]
    g = m.open_stream_group(3, window=T, stride=stride, max_push=2)
    assert (g.cap, g.total_slots) == (CAP, 3 * CAP)
    lone = [m.open_stream(window=T, stride=stride, max_push=2) for _ in range(3)]
    seen = [0, 0, 0]
    began = [set(), set(), set()]   # the ring slots at which a camera's pushes began
    at_end = [set(), set(), set()]  # which frame of a window lay in the ring's last slot, where the window wraps
    per_camera, per_lone, silent = [[], [], []], [[], [], []], 0
    for ks in PUSHES:
        outs = g.push(entries(xs, seen, ks))
        assert len(outs) == 3
        clips = []
        for s, k in enumerate(ks):
            k = k or 0
            want = completed(seen[s], k, stride)
            assert outs[s]["window_starts"].dtype == torch.int64 and outs[s]["window_starts"].tolist() == want
            assert all(outs[s][key].shape[0] == len(want) for key in KEYS[kind])
            if k:
                began[s].add(seen[s] % CAP)
                per_lone[s].append(lone[s].push(xs[s][seen[s]:seen[s] + k]))
            for w in want:
                if w % CAP + T > CAP:
                    at_end[s].add(CAP - 1 - w % CAP)
            if want:
                clips.append(gather(xs[s], T, want))
            per_camera[s].append(outs[s])
            seen[s] += k
        if clips:
            n = sum(c.shape[0] for c in clips)
            assert n <= 6
            assert_same(kind, dict(zip(KEYS[kind], cat_cameras(kind, outs))), clip_call(kind, m, torch.cat(clips)),
                        f"push {ks} ending at frames {seen}")
        else:
            silent += 1
            assert all(empty(kind, o) for o in outs)
    assert silent == (1 if stride == 1 else 4)
    assert began == [set(range(CAP))] * 3 and at_end == [{0, 1, 2}] * 3
    assert g.frames_seen == TOTAL and g.windows_emitted == [(n - T) // stride + 1 for n in TOTAL]
    assert g._ring.shape == (3 * CAP, C, H, W)
    for s in range(3):
        got = {k: torch.cat([o[k] for o in per_camera[s]]) for k in KEYS[kind] + ("window_starts",)}
        assert got["window_starts"].tolist() == list(range(0, TOTAL[s] - T + 1, stride))
        assert_same(kind, got, cat_cameras(kind, per_lone[s]), f"camera {s} against a lone ClipStream")
        assert got["anomaly_scores"].unique().numel() > 1
        assert torch.equal(g._ring[s * CAP:(s + 1) * CAP], lone[s]._ring)


@pytest.mark.parametrize("kind", KINDS)
def test_a_push_that_completes_no_window_calls_nothing(kind):
    """Frames are scattered to their slots and every camera gets empty device tensors: the library is not called (a call
    with nw = 0 would be refused), and the next push scores from the right slots."""
    m = make(kind)
    C = CHANNELS[kind]
    xs = [video(70 + s, 9, C, H, W) for s in range(2)]
    g = m.open_stream_group(2, window=T, stride=3, max_push=3)
    g.push([xs[0][0:3], xs[1][0:2]])
    eng = m.scoring_engine(xs[0].device)
    calls = []
    real = eng.windows_forward_group
    eng.windows_forward_group = lambda *a, **kw: (calls.append(a[3]), real(*a, **kw))[1]
    try:
        a = g.push([xs[0][3:4], xs[1][2:3]])   # camera 0: frames 0..3, window 0; camera 1 has three frames
        b = g.push([xs[0][4:6], None])         # camera 0: frames 4, 5 -- window 3 needs frame 6
        c = g.push([xs[0][6:9], xs[1][3:6]])   # camera 0: window 3; camera 1: window 0 (window 3 needs frame 6)
    finally:
        del eng.windows_forward_group
    assert calls == [1, 2]
    assert [o["window_starts"].tolist() for o in a] == [[0], []] and empty(kind, a[1])
    assert empty(kind, b[0]) and empty(kind, b[1])
    assert [o["window_starts"].tolist() for o in c] == [[3], [0]]
    assert g.frames_seen == [9, 6] and g.windows_emitted == [2, 1]
    want = clip_call(kind, m, torch.cat([gather(xs[0], T, [3]), gather(xs[1], T, [0])]))
    assert_same(kind, dict(zip(KEYS[kind], cat_cameras(kind, c))), want)


@pytest.mark.parametrize("kind", KINDS)
def test_reset_restarts_one_camera_and_leaves_the_others(kind):
    m = make(kind)
    C = CHANNELS[kind]
    xs = [video(80 + s, 12, C, H, W) for s in range(3)]
    again = video(83, 6, C, H, W)  # what camera 1 shows after its reset
    g = m.open_stream_group(3, window=T, stride=1, max_push=2)
    lone = [m.open_stream(window=T, stride=1, max_push=2) for _ in range(3)]
    for f in range(0, 12, 2):
        if f == 6:
            g.reset(1)
            lone[1].reset()
            assert g.frames_seen == [6, 0, 6] and g.windows_emitted == [3, 0, 3]
        src = [xs[0], again if f >= 6 else xs[1], xs[2]]
        f1 = f - 6 if f >= 6 else f
        outs = g.push([src[0][f:f + 2], src[1][f1:f1 + 2], src[2][f:f + 2]])
        want = [lone[0].push(src[0][f:f + 2]), lone[1].push(src[1][f1:f1 + 2]), lone[2].push(src[2][f:f + 2])]
        for s in range(3):
            assert outs[s]["window_starts"].tolist() == want[s]["window_starts"].tolist()
            assert_same(kind, outs[s], want[s], f"camera {s} at frame {f}")
        if f == 8:  # camera 1 counts from its reset: its frames 0..3 again, scored from the new frames
            assert outs[1]["window_starts"].tolist() == [0] and outs[0]["window_starts"].tolist() == [5, 6]
            assert_same(kind, outs[1], clip_call(kind, m, gather(again, T, [0])))
    assert g.frames_seen == [12, 6, 12] and g.windows_emitted == [9, 3, 9]
    g.reset()
    assert g.frames_seen == [0, 0, 0] and g.windows_emitted == [0, 0, 0]


def camera(seed, k, Hs, Ws, C):
    shape = (k, Hs, Ws) if C == 1 else (k, Hs, Ws, 3)
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("kind, color", [("mc1", None), ("mc1", "bgr"), ("a2", "bgr"), ("bbox", "bgr")],
                         ids=["mc1-grey", "mc1-bgr-luma", "a2-bgr", "bbox-bgr"])
def test_push_u8_is_push_of_ingest_u8(kind, color):
    """Three cameras of three source sizes: camera 0's frames on the device, camera 1's in pinned host memory, camera
    2's in pageable host memory.  One table-form ingest launch per push against data.ingest_u8 per camera."""
    C = CHANNELS[kind]
    m = make(kind)
    sizes = [(20, 31), (17, 13), (40, 22)]
    u8 = [camera(90 + s, 8, *sizes[s], 1 if color is None else 3) for s in range(3)]
    place = [lambda t: t.cuda(), lambda t: t.pin_memory(), lambda t: t]
    a = m.open_stream_group(3, window=T, stride=1, max_push=2, frame_size=(H, W))
    b = m.open_stream_group(3, window=T, stride=1, max_push=2, frame_size=(H, W))
    seen = [0, 0, 0]
    keep = []  # (pinned sources are read in place: they stay alive until the device is idle)
    for i, ks in enumerate([(2, 2, 1), (2, 1, 2), (1, None, 2), (2, 2, 2), (1, 2, 1)]):
        raw = [None if k is None else u8[s][seen[s]:seen[s] + k] for s, k in enumerate(ks)]
        placed = [None if r is None else place[s](r) for s, r in enumerate(raw)]
        keep.append(placed)
        assert placed[1] is None or placed[1].is_pinned()
        got = a.push_u8(placed, color=color)
        want = b.push([None if r is None else data.ingest_u8(r.cuda(), (H, W), 1, color=color, planes=C) for r in raw])
        for s, k in enumerate(ks):
            seen[s] += k or 0
            assert got[s]["window_starts"].tolist() == want[s]["window_starts"].tolist()
            assert_same(kind, got[s], want[s], f"push {i} camera {s}")
        assert torch.equal(a._ring, b._ring)
    assert a.frames_seen == b.frames_seen == [8, 7, 8]
    assert got[0]["window_starts"].tolist() == [4] and got[1]["window_starts"].tolist() == [2, 3]
    assert a._u8.shape == (6, C, H, W) and b._u8 is None
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", KINDS)
def test_group_at_64x64_with_the_model_s_default_window(kind):
    m = make(kind, T=4)
    Tw = 8 if kind == "a2" else 4
    C = CHANNELS[kind]
    xs = [video(100 + s, Tw + 4, C, 64, 64) for s in range(2)]
    g = m.open_stream_group(2, stride=2, max_push=2)
    assert g.window == Tw and g.cap == Tw + 1
    f = [0, 0]
    for i in range(Tw // 2 + 2):
        ks = (2, 2) if i % 3 else (2, 1)  # camera 1 falls a frame behind twice
        outs = g.push(entries(xs, f, ks))
        clips = []
        for s in range(2):
            want = completed(f[s], ks[s], 2, Tw)
            f[s] += ks[s]
            assert outs[s]["window_starts"].tolist() == want
            if want:
                clips.append(gather(xs[s], Tw, want))
        if clips:
            assert_same(kind, dict(zip(KEYS[kind], cat_cameras(kind, outs))), clip_call(kind, m, torch.cat(clips)))
    assert g.windows_emitted[0] >= 3 and g.windows_emitted[1] >= 2


@pytest.mark.parametrize("kind", KINDS)
def test_state_is_unchanged_and_a_group_and_a_stream_share_the_model(kind):
    """The model's state_dict -- parameters, BatchNorm running statistics and counters -- is bit-identical after a group
    run, and a group and a ClipStream pushed in turn on one model give what each gives alone."""
    m = make(kind)
    C = CHANNELS[kind]
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    xs = [video(110 + s, 10, C, H, W) for s in range(3)]

    def run_group(between=None):
        g = m.open_stream_group(2, window=T, stride=1, max_push=2)
        outs = []
        for f in range(0, 10, 2):
            outs.append(g.push([xs[0][f:f + 2], xs[1][f:f + 2]]))
            if between is not None:
                between(f)
        return [cat_cameras(kind, [o[s] for o in outs]) for s in range(2)]

    def run_stream(st):
        return cat_cameras(kind, [st.push(xs[2][f:f + 2]) for f in range(0, 10, 2)])

    alone_g = run_group()
    alone_s = run_stream(m.open_stream(window=T, stride=1, max_push=2))
    st, mixed_s = m.open_stream(window=T, stride=1, max_push=2), []
    mixed_g = run_group(lambda f: mixed_s.append(st.push(xs[2][f:f + 2])))
    for s in range(2):
        assert all(torch.equal(a, b) for a, b in zip(alone_g[s], mixed_g[s]))
    assert all(torch.equal(a, b) for a, b in zip(alone_s, cat_cameras(kind, mixed_s)))
    after = m.state_dict()
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)


SENTINEL = 0x5A5A5A5A


@pytest.mark.parametrize("kind", ["a2", "mc1", "bbox"])
def test_group_entry_points_refuse_bad_arguments_and_queue_nothing(kind):
    """vad_a2 / vad_mc / vad_bbox _windows_forward_group: a bad base, first >= cap, nw outside 1..B, cap < T and a null
    table return non-zero with a text that names the entry point and the numbers; no output, no table word and no ring
    word is written.  The same call with a legal table then runs."""
    m = make(kind)
    C = CHANNELS[kind]
    L = nat.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    eng = m.scoring_engine(dev)
    B, cap, slots = 2, CAP, 2 * CAP
    pfx = {"a2": "a2", "mc1": "mc", "bbox": "bbox"}[kind]
    fn = getattr(L, f"vad_{pfx}_windows_forward_group")
    pl = eng.plan(B, C, T, H, W) if kind == "bbox" else eng.plan(B, C, T, H, W, "windows")
    assert L.vad_win_group_table_bytes(1) == 32 and L.vad_win_group_table_bytes(5) == 80
    assert L.vad_win_group_table_bytes(0) == -1 and b"vad_win_group_table_bytes" in L.vad_last_error()
    ring = video(120, slots, C, H, W)
    ring0 = ring.clone()
    table = torch.full((L.vad_win_group_table_bytes(B) // 4,), SENTINEL, dtype=torch.int32, device=dev)
    outs = [torch.full_like(o, 7.0) for o in eng.window_outputs(B)]
    st = nat.stream_of(dev)
    host = []  # (the host tables stay alive until the device is idle)
    ok = ((0, 3), (5, 1))

    def call(rows=ok, nw=None, cap_=cap, slots_=slots, host_table=True, dev_table=True, plan=pl.h):
        host.append(torch.tensor(rows, dtype=torch.int64))
        return fn(plan, ring.data_ptr(), slots_, cap_, host[-1].data_ptr() if host_table else None,
                  len(rows) if nw is None else nw, table.data_ptr() if dev_table else None,
                  *[o.data_ptr() for o in outs], st)

    for refused, text in [
            (lambda: call(((0, 3), (3, 0))), b"window 1 (base 3, first 0): base must be a non-negative multiple of cap"),
            (lambda: call(((-5, 0), (5, 1))), b"window 0 (base -5, first 0): base must be a non-negative multiple"),
            (lambda: call(((0, 3), (10, 0))), b"window 1 (base 10, first 0): base + cap exceeds total_slots"),
            (lambda: call(((0, 3), (5, cap))), b"window 1 (base 5, first 5): first must be in 0..cap - 1"),
            (lambda: call(((0, -1), (5, 1))), b"window 0 (base 0, first -1): first must be in 0..cap - 1"),
            (lambda: call(nw=0), b"between 1 and the plan's 2 windows per call, got 0"),
            (lambda: call(ok + ((0, 0),)), b"between 1 and the plan's 2 windows per call, got 3"),
            (lambda: call(((0, 0), (3, 0)), cap_=3, slots_=6), b"a ring of cap = 3 slots holds no window of 4 frames"),
            (lambda: call(cap_=0), b"cap must be in 1..total_slots and divide it, got cap 0, total_slots 10"),
            (lambda: call(slots_=slots + 1), b"cap must be in 1..total_slots and divide it, got cap 5, total_slots 11"),
            (lambda: call(host_table=False), b"null table"),
            (lambda: call(dev_table=False), b"null table"),
            (lambda: call(plan=None), b"null plan")]:
        assert refused() != 0
        err = L.vad_last_error()
        assert f"vad_{pfx}_windows_forward_group".encode() in err and text in err, err
    if kind == "bbox":  # the whole plan runs
        assert call(ok[:1]) != 0 and b"nw must be its 2 windows, got 1" in L.vad_last_error()
    torch.cuda.synchronize()
    assert bool((table == SENTINEL).all()) and torch.equal(ring, ring0)
    assert all(bool((o == 7.0).all()) for o in outs)
    assert call() == 0
    torch.cuda.synchronize()
    rows = torch.tensor(ok, dtype=torch.int64)
    assert torch.equal(table.view(torch.int64)[:4].cpu(), rows.reshape(-1))
    frames = [[b + (f + t) % cap for t in range(T)] for b, f in ok]
    clips = torch.stack([ring[idx].permute(1, 0, 2, 3) for idx in frames]).contiguous()
    assert_same(kind, dict(zip(KEYS[kind], outs)), clip_call(kind, m, clips))
    if kind == "a2":  # a single window: row 0 twice, row 0 returned; the second output row is left alone
        keep = [o[1].clone() for o in outs]
        assert call(ok[1:]) == 0
        torch.cuda.synchronize()
        assert_same(kind, {k: o[:1] for k, o in zip(KEYS[kind], outs)}, clip_call(kind, m, clips[1:]))
        assert all(torch.equal(o[1], k) for o, k in zip(outs, keep))
