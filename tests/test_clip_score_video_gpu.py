"""a2 / minicausal score_video on the GPU (bbox's has its own file): the first conv reads every window in place, the
rest of the forward is the clip path's on the same number of clips, so a batch of windows must come out bit for bit as
``model(clips)`` has it for those windows gathered with torch into one batch of the same size -- the criterion of
test_bbox_score_video_gpu.py.  a2 cannot run one clip (its plans hold at least two), so a single window is held against
``model(torch.stack([clip, clip]))`` row 0.  Shapes are the smallest at which the addressing can go wrong: 10 x 13
frames (odd, ragged against every tile), windows of 4 (a2 also 8, and 1: the shortest clip vad_a2_create takes), a
stride that does not divide N - window, a ragged last batch, a batch of one; 64 x 64 once per model."""
import pytest
import torch

from vad_amd import _native as nat

pytestmark = pytest.mark.gpu

KINDS = ("a2", "mc1", "mc3", "bbox")
CHANNELS = {"a2": 3, "mc1": 1, "mc3": 3, "bbox": 3}
KEYS = {"a2": ("anomaly_scores", "causal_graphs", "features"), "mc1": ("anomaly_scores",), "mc3": ("anomaly_scores",),
        "bbox": ("anomaly_scores", "causal_graphs", "features")}


def make(kind, seed=5, T=4):
    """The model on the device in eval mode.  minicausal: non-trivial BatchNorm state (random running statistics and
    affine parameters) and a classifier wide enough for the scores to tell windows apart (its init, N(0, 0.01), gives
    0.5 for everything)."""
    torch.manual_seed(seed)
    if kind == "a2":
        from vad_amd.a2 import CausalAnomalyDetector
        return CausalAnomalyDetector().cuda().eval()
    if kind == "bbox":
        from vad_amd.bbox import CausalAnomalyDetector
        return CausalAnomalyDetector(num_frames=T).cuda().eval()
    from vad_amd.mc import SimpleVideoAnomalyDetector
    m = SimpleVideoAnomalyDetector(input_channels=CHANNELS[kind], temporal_frames=T)
    sd = m.state_dict()
    for k, v in sd.items():
        if k.endswith("running_var"):
            sd[k] = torch.rand_like(v) + 0.5
        elif k.endswith("running_mean"):
            sd[k] = torch.randn_like(v) * 0.3
        elif k.startswith("features") and v.dim() == 1 and k.endswith("weight"):
            sd[k] = torch.rand_like(v) + 0.5
        elif k.startswith("features") and v.dim() == 1 and k.endswith("bias"):
            sd[k] = torch.randn_like(v) * 0.2
        elif k.startswith("classifier"):
            sd[k] = torch.randn_like(v) * 0.7
    m.load_state_dict(sd)
    return m.cuda().eval()


def video(seed, N, C, H, W):
    return torch.rand(N, C, H, W, generator=torch.Generator().manual_seed(seed)).cuda()


def gather(x, window, starts):
    """The clips (Wn, C, T, H, W) of the windows of x (N, C, H, W) that start at `starts`, copied with torch."""
    return torch.stack([x[s:s + window].permute(1, 0, 2, 3) for s in starts]).contiguous()


def clip_call(kind, m, clips):
    """model(clips) for one batch -> the outputs in KEYS order, scores as (n,); a2 with one clip: the clip twice."""
    n = clips.shape[0]
    if kind == "a2" and n == 1:
        clips = torch.cat([clips, clips])
    with torch.no_grad():
        o = m(clips)
    o = (o,) if isinstance(o, torch.Tensor) else tuple(o)
    return tuple(t.reshape(-1)[:n].clone() if i == 0 else t[:n].clone() for i, t in enumerate(o))


def clip_path(kind, m, clips, batch):
    parts = [clip_call(kind, m, clips[w0:w0 + batch]) for w0 in range(0, clips.shape[0], batch)]
    return tuple(torch.cat(t) for t in zip(*parts))


def assert_same(kind, got, want, what=""):
    """got: a result dict; want: another, or the outputs in KEYS order."""
    if isinstance(want, dict):
        want = tuple(want[k] for k in KEYS[kind])
    for k, w in zip(KEYS[kind], want):
        assert got[k].shape == w.shape, (what, k, got[k].shape, w.shape)
        assert torch.equal(got[k], w), (what, k, float((got[k] - w).abs().max()))


def model_state(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


CASES = [
    # N, window, stride, batch, H, W
    (13, 4, 1, 4, 10, 13),    # 10 windows: 4 + 4 + 2, the last batch ragged (a2: nw = 2 on the plan of 4)
    (13, 4, 3, 64, 10, 13),   # windows at 0, 3, 6, 9 in one batch
    (13, 4, 3, 1, 10, 13),    # a batch of one (a2: the plan of two, nw = 1)
    (14, 4, 3, 3, 10, 13),    # stride 3 does not divide N - window = 10: frame 13 is in no window; 3 + 1
    (4, 4, 1, 64, 10, 13),    # N == window: a single window
    (12, 4, 2, 3, 64, 64),    # 5 windows, 3 + 2, at 64 x 64
]


@pytest.mark.parametrize("kind", KINDS[:3])
@pytest.mark.parametrize("N, window, stride, batch, H, W", CASES,
                         ids=[f"N{c[0]}-T{c[1]}-s{c[2]}-b{c[3]}-{c[4]}x{c[5]}" for c in CASES])
def test_score_video_is_the_clip_path(kind, N, window, stride, batch, H, W):
    m = make(kind)
    before = model_state(m)
    x = video(N * 10 + stride, N, CHANNELS[kind], H, W)
    starts = list(range(0, N - window + 1, stride))
    o = m.score_video(x, window=window, stride=stride, batch=batch)
    assert o["window_starts"].dtype == torch.int64 and o["window_starts"].tolist() == starts
    assert o["anomaly_scores"].shape == (len(starts),)
    assert_same(kind, o, clip_path(kind, m, gather(x, window, starts), batch))
    if len(starts) > 1:  # the check can tell windows apart
        assert o["anomaly_scores"].unique().numel() > 1
    after = model_state(m)  # parameters, running_mean, running_var, num_batches_tracked: bit-identical
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)


@pytest.mark.parametrize("window, N, stride, batch", [(8, 13, 2, 2), (1, 5, 2, 2), (1, 1, 1, 1)],
                         ids=["T8", "T1-shortest-clip", "T1-single-frame"])
def test_a2_window_lengths(window, N, stride, batch):
    m = make("a2")
    x = video(window, N, 3, 10, 13)
    starts = list(range(0, N - window + 1, stride))
    o = m.score_video(x, window=window, stride=stride, batch=batch)
    assert_same("a2", o, clip_path("a2", m, gather(x, window, starts), batch))


@pytest.mark.parametrize("kind", KINDS[:3])
def test_non_contiguous_frames_are_made_contiguous(kind):
    m = make(kind)
    C = CHANNELS[kind]
    wide = video(3, 9, C, 10, 26)
    x = wide[:, :, :, ::2]                       # every other column: strided rows
    t = video(4, 9, C, 13, 10).transpose(2, 3)   # (9, C, 10, 13) with H and W swapped in memory
    for v in (x, t):
        assert not v.is_contiguous()
        assert_same(kind, m.score_video(v, window=4, stride=2), m.score_video(v.contiguous(), window=4, stride=2))
    starts = [0, 2, 4]
    assert_same(kind, m.score_video(x, window=4, stride=2), clip_path(kind, m, gather(x, 4, starts), 64))


def test_mc_defaults_and_a2_defaults():
    m = make("mc1", T=4)
    x = video(8, 13, 1, 10, 13)
    o = m.score_video(x)  # window = temporal_frames = 4, stride 4
    assert o["window_starts"].tolist() == [0, 4, 8]
    assert_same("mc1", o, m.score_video(x, window=4, stride=4, batch=64))
    a = make("a2")
    assert a.score_video(video(9, 17, 3, 10, 13))["window_starts"].tolist() == [0, 4, 8]  # window 8, stride 4


def test_a2_train_step_is_not_disturbed_by_score_video():
    """train_step -> score_video -> train_step on one trainer against two train_steps on a fresh identical one."""
    from vad_amd.a2 import ImprovedMiniCausalVAD
    clips = [torch.rand(4, 3, 4, 10, 13, generator=torch.Generator().manual_seed(s)) for s in (1, 2)]
    x = video(3, 13, 3, 10, 13)
    runs = []
    for score in (True, False):
        torch.manual_seed(11)
        tr = ImprovedMiniCausalVAD(device="cuda")
        l0 = tr.train_step(clips[0], None)
        if score:
            tr.model.eval()
            tr.model.score_video(x, window=4, stride=1, batch=4)  # the train step's own shape: (4, 3, 4, 10, 13)
        l1 = tr.train_step(clips[1], None)
        runs.append((l0[0], l1[0], tr.model.feature_extractor.conv3d_1.weight.detach().clone(),
                     tr.model.anomaly_predictor[0].weight.detach().clone()))
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    assert torch.equal(runs[0][2], runs[1][2]) and torch.equal(runs[0][3], runs[1][3])


def test_mc_train_step_is_not_disturbed_by_score_video():
    from vad_amd.mc import SimpleVideoAnomalyDetector, StableTrainer
    g = torch.Generator().manual_seed(1)
    data = [torch.rand(4, 1, 4, 10, 13, generator=g) for _ in range(2)]
    y = torch.tensor([0., 1., 1., 0.])
    x = video(3, 13, 1, 10, 13)
    runs = []
    for score in (True, False):
        torch.manual_seed(12)
        tr = StableTrainer(SimpleVideoAnomalyDetector(input_channels=1, temporal_frames=4), None, None, "cuda")
        l0 = tr.train_step(data[0], y)
        if score:
            tr.model.eval()
            tr.model.score_video(x, window=4, stride=1, batch=4)
        l1 = tr.train_step(data[1], y)
        runs.append((l0[0], l1[0], model_state(tr.model)))
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    assert all(torch.equal(runs[0][2][k], runs[1][2][k]) for k in runs[0][2])  # BatchNorm buffers and counters too


@pytest.mark.parametrize("kind", ["a2", "mc1"])
def test_score_video_between_a_forward_and_its_backward_leaves_the_backward_unchanged(kind):
    """score_video runs on scoring plans of its own, so a backward pending on a training forward of the same shape
    gives the gradients it gives undisturbed."""
    x = video(5, 13, CHANNELS[kind], 10, 13)
    clips = gather(x, 4, [0, 3, 6, 9])
    grads = []
    for score in (True, False):
        m = make(kind, seed=21)
        m.train()
        o = m(clips, seed=7, step=0)
        s = o if isinstance(o, torch.Tensor) else o[0]
        if score:
            m.eval()
            m.score_video(x, window=4, stride=3, batch=4)  # 4 windows: the pending forward's very shape
            m.train()
        s.sum().backward()
        grads.append([p.grad.detach().clone() for p in m.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*grads))
    assert any(float(g.abs().max()) > 0 for g in grads[0])


@pytest.mark.parametrize("kind", ["a2", "mc1"])
def test_windows_call_on_a_plan_with_a_pending_backward_makes_the_backward_raise(kind):
    """The entry point itself, called on the training plan: it overwrites the activations, and the backward says so
    instead of using them; the next clip forward clears it."""
    m = make(kind, seed=22)
    x = video(6, 13, CHANNELS[kind], 10, 13)
    clips = gather(x, 4, [0, 3, 6, 9])
    m.train()
    o = m(clips, seed=7, step=0)
    e = m._engine
    L = nat.lib()
    scores = torch.empty(4, device="cuda")
    if kind == "a2":
        nat.check(L.vad_a2_windows_forward(e.cur.h, x.data_ptr(), 13, 0, 3, 0, 4, scores.data_ptr(), None, None,
                                           e.stream()))
    else:
        nat.check(L.vad_mc_windows_forward(e.cur.h, x.data_ptr(), 13, 0, 3, 0, 4, scores.data_ptr(), e.stream()))
    m.eval()
    assert torch.equal(scores, m.score_video(x, window=4, stride=3)["anomaly_scores"])
    m.train()
    s = o if isinstance(o, torch.Tensor) else o[0]
    with pytest.raises(RuntimeError, match="has overwritten this plan's activations"):
        s.sum().backward()
    o = m(clips, seed=7, step=0)
    (o if isinstance(o, torch.Tensor) else o[0]).sum().backward()  # a fresh forward: the backward runs again
    torch.cuda.synchronize()
