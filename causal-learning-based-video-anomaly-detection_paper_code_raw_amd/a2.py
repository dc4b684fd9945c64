"""Drop-in for avenue_training_script2.py: the a2 CausalAnomalyDetector (a2:15-101) and ImprovedMiniCausalVAD
(a2:107-297) with forward / loss / backward / AdamW on the HIP plan (``vad_a2_*`` in libvadhip.so).

Same class names, constructor signatures, submodule names (state_dict keys ``feature_extractor.conv3d_1.weight``
... so the reference's ``best_improved_model.pth`` loads strictly), initialisation order and forward return
``(scores (B,1), causal_adj (B,16,16), features (B,16))``.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _native as nat
from ._flat import FlatEngine, FlatPlan


class CompactFeatureExtractor(nn.Module):
    """a2:15-35"""

    def __init__(self, input_channels=3, feature_dim=64):
        super().__init__()
        self.conv3d_1 = nn.Conv3d(input_channels, 16, (3, 3, 3), stride=(1, 2, 2), padding=1)
        self.conv3d_2 = nn.Conv3d(16, 32, (3, 3, 3), stride=(2, 2, 2), padding=1)
        self.conv3d_3 = nn.Conv3d(32, 64, (3, 3, 3), stride=(2, 2, 2), padding=1)
        self.adaptive_pool = nn.AdaptiveAvgPool3d((4, 4, 4))
        self.fc = nn.Linear(64 * 4 * 4 * 4, feature_dim)
        self.dropout = nn.Dropout(0.3)


class DifferentiableCausalDiscovery(nn.Module):
    """a2:37-66"""

    def __init__(self, num_variables=16, hidden_dim=32):
        super().__init__()
        self.num_variables = num_variables
        self.causal_net = nn.Sequential(nn.Linear(num_variables, hidden_dim), nn.ReLU(),
                                        nn.Linear(hidden_dim, num_variables * num_variables), nn.Sigmoid())

    def acyclicity_constraint(self, adj_matrix):
        """a2:62-66 (host-side helper, unchanged semantics)."""
        m = adj_matrix.mean(dim=0)
        return torch.trace(torch.matrix_power(m + 1e-8, 2))


class CausalAnomalyDetector(nn.Module):
    """a2:69-101.  forward(video_clips (B,3,T,H,W)) -> (anomaly_scores (B,1), causal_adj (B,16,16), features (B,16))."""

    def __init__(self, feature_dim=64, causal_dim=16, hidden_dim=128):
        super().__init__()
        self.feature_extractor = CompactFeatureExtractor(feature_dim=causal_dim)
        self.causal_discovery = DifferentiableCausalDiscovery(num_variables=causal_dim)
        self.graph_encoder = nn.Sequential(nn.Linear(causal_dim * causal_dim, hidden_dim), nn.ReLU(), nn.Dropout(0.3),
                                           nn.Linear(hidden_dim, 64))
        self.anomaly_predictor = nn.Sequential(nn.Linear(causal_dim + 64, 32), nn.ReLU(), nn.Linear(32, 1),
                                               nn.Sigmoid())
        self._engine = None
        self._step = 0

    def engine(self, x: torch.Tensor) -> "A2Engine":
        e = self._engine
        if e is None or e.device != x.device:
            e = A2Engine(self, x.device)
            self._engine = e
        e.use_shape(tuple(x.shape))
        return e

    def forward(self, video_clips, *, seed=None, step=None, clip0=0):
        if video_clips.dim() != 5 or video_clips.shape[1] != 3:
            raise ValueError(f"Expected (B,3,T,H,W) clips, got {tuple(video_clips.shape)}")
        nat.require_hip(video_clips)
        x = video_clips.float().contiguous()
        e = self.engine(x)
        if seed is None:
            seed = e.seed
        if step is None:
            step = self._step
            if self.training:
                self._step += 1
        e.last_keys = (seed, step, clip0)
        params = [p for _, p in self.named_parameters()]
        return _A2Function.apply(x, e, self.training, seed, step, clip0, *params)

    def scoring_engine(self, device) -> "A2Engine":
        """The engine on `device`, made if need be, without choosing a clip plan (score_video, open_stream)."""
        e = self._engine
        if e is None or e.device != device:
            e = self._engine = A2Engine(self, device)
        return e

    def score_video(self, frames, window=8, stride=4, batch=64) -> dict:
        """Score every full window ``range(0, N - window + 1, stride)`` of a video: frames fp32 (N, 3, H, W) on the
        device, planar RGB (``data.ingest_u8(u8, (64, 64), 1, color=..., planes=3)`` builds them from camera bytes).
        Windows run ``batch`` at a time and are never copied into clips: conv3d_1 reads window b's frames in place
        (``vad_a2_windows_forward``).  Returns anomaly_scores (W,), causal_graphs (W, 16, 16), features
        (W, 16) -- for the windows of one batch what ``model(clips)`` returns in eval mode for those windows gathered
        into (3, T, H, W) clips, a single window as ``model(torch.stack([clip, clip]))`` row 0 -- and window_starts (W,)
        int64 on the host.  Eval mode only; runs on plans of its own, so a pending backward is not disturbed."""
        from .clip_stream import check_score_video, score_video
        x = check_score_video("a2", self, frames, window, stride, batch)
        nat.require_hip(x)
        return score_video(self.scoring_engine(x.device), x.float().contiguous(), int(window), int(stride), int(batch))

    def open_stream(self, window=8, stride=1, *, max_push=1, frame_size=None):
        """A clip_stream.ClipStream on this model: push frames (k, 3, H, W) as they arrive, get score_video's keys for
        the windows they complete, read from a ring of window + max_push - 1 raw frames."""
        from .clip_stream import ClipStream
        return ClipStream(self, "a2", window, stride, max_push=max_push, frame_size=frame_size)

    def open_stream_group(self, num_streams, window=8, stride=1, *, max_push=1, frame_size=None):
        """A clip_stream_group.ClipStreamGroup on this model: num_streams cameras of one frame size, one windows call
        per push for the windows of all of them."""
        from .clip_stream_group import ClipStreamGroup
        return ClipStreamGroup(self, "a2", num_streams, window, stride, max_push=max_push, frame_size=frame_size)


class _A2Function(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, e, training, seed, step, clip0, *params):
        s, adj, f = e.forward(x, training, seed, step, clip0, with_loss=False)
        ctx.e = e
        return s.view(-1, 1).clone(), adj.clone(), f.clone()

    @staticmethod
    def backward(ctx, d_s, d_adj, d_f):
        e = ctx.e
        e.backward(None if d_s is None else d_s.reshape(-1).contiguous().float(),
                   None if d_adj is None else d_adj.contiguous().float(),
                   None if d_f is None else d_f.contiguous().float())
        return (None, None, None, None, None, None, *e.grad_clones())


class _A2LossFunction(torch.autograd.Function):
    """compute_improved_loss on the engine's last forward; backward hands d total / d (scores, adj) upstream."""

    @staticmethod
    def forward(ctx, scores, adj, e, seed, step, clip0):
        e.loss(seed, step, clip0)
        ctx.e = e
        return e.losses[0].clone()

    @staticmethod
    def backward(ctx, g):
        ds, dadj = ctx.e.loss_grads()
        return (ds.view(-1, 1) * g, dadj * g, None, None, None, None)


class _A2Plan(FlatPlan):
    def __init__(self, e, B, C, T, H, W, *tag):  # tag ("windows",): a scoring plan, apart from the clip plan of its shape
        super().__init__(e, B, C, T, H, W, *tag)
        self.B = B
        f = dict(dtype=torch.float32, device=e.device)
        self.scores, self.adj, self.feats = torch.zeros(B, **f), torch.zeros(B, 16, 16, **f), torch.zeros(B, 16, **f)
        self.d_s, self.d_adj = torch.zeros(B, **f), torch.zeros(B, 16, 16, **f)
        self.borrow = False

    @staticmethod
    def create_args(B, C, T, H, W, *tag):
        return B, T, H, W


class A2Engine(FlatEngine):
    """Flat device buffers (params / grads / AdamW state, named_parameters order) shared by per-shape plans."""
    PLAN = _A2Plan

    def __init__(self, model, device):
        super().__init__(model, device, "a2", replace_params=True, opt_state="eager",
                         bind_names=("params", "grads", "exp_avg", "exp_avg_sq", "steps"),
                         name_mismatch=(NotImplementedError, "the HIP a2 plan supports the reference dims "
                                        "(feature_dim=64, causal_dim=16, hidden_dim=128) only"))
        self.seed, self.last_keys = 1234, (0, 0, 0)
        self.losses = torch.zeros(10, dtype=torch.float32, device=device)

    def use_shape(self, shape):
        self.cur = self.plan(*shape)

    def forward(self, x, training, seed, step, clip0, with_loss, borrow_input=False):
        """borrow_input: x stays unchanged until the backward (the fused train step): conv3d_1 reads it in place."""
        p = self.cur
        if p.borrow != bool(borrow_input):
            nat.check(nat.lib().vad_a2_set_option(p.h, b"borrow_input", int(bool(borrow_input))))
            p.borrow = bool(borrow_input)
        nat.check(nat.lib().vad_a2_forward(p.h, nat.ptr(x), int(training), ctypes.c_uint64(seed),
                                           ctypes.c_uint64(step), ctypes.c_int64(clip0), int(with_loss),
                                           nat.ptr(p.scores), nat.ptr(p.adj), nat.ptr(p.feats),
                                           nat.ptr(self.losses) if with_loss else None, self.stream()))
        return p.scores, p.adj, p.feats

    WINDOW_KEYS = ("anomaly_scores", "causal_graphs", "features")

    def window_outputs(self, n):
        f = dict(dtype=torch.float32, device=self.device)
        return torch.empty(n, **f), torch.empty(n, 16, 16, **f), torch.empty(n, 16, **f)

    def windows_forward(self, frames, first, stride, ring, nw, T, B, out):
        """nw <= B windows of frames (n, 3, H, W) -- a video (ring 0) or a ring of `ring` slots -- into the tensors
        out (window_outputs' order).  The plan holds max(B, 2) clips (vad_a2_create) and is a scoring plan: no clip
        forward runs on it, so no backward can be pending on the activations it overwrites."""
        n, _, H, W = frames.shape
        p = self.plan(max(B, 2), 3, T, H, W, "windows")
        nat.check(nat.lib().vad_a2_windows_forward(p.h, nat.ptr(frames), n, first, stride, ring, nw, *map(nat.ptr, out),
                                                   self.stream()))

    def windows_forward_group(self, ring, cap, h_win, nw, dev_table, T, B, out):
        """nw <= B windows of a group's rings (total_slots, 3, H, W), cap slots each, through the host rows h_win
        (nw, 2) int64 and the caller's device table (vad_a2_windows_forward_group), into the tensors out; on
        windows_forward's scoring plan."""
        n, _, H, W = ring.shape
        p = self.plan(max(B, 2), 3, T, H, W, "windows")
        nat.check(nat.lib().vad_a2_windows_forward_group(p.h, nat.ptr(ring), n, cap, h_win.data_ptr(), nw,
                                                         nat.ptr(dev_table), *map(nat.ptr, out), self.stream()))

    def set_host_losses(self, buf):
        """Let the current plan's forward also write its 10 loss words into `buf` (a pinned CPU tensor; None: stop)."""
        p = self.cur
        ptr = buf.data_ptr() if buf is not None else 0
        if getattr(p, "host_ptr", 0) != ptr:
            nat.check(nat.lib().vad_a2_set_option(p.h, b"host_losses", ctypes.c_int64(ptr)))
            p.host_ptr = ptr

    def loss(self, seed, step, clip0):
        nat.check(nat.lib().vad_a2_loss(self.cur.h, ctypes.c_uint64(seed), ctypes.c_uint64(step),
                                        ctypes.c_int64(clip0), nat.ptr(self.losses), self.stream()))

    def loss_grads(self):
        p = self.cur
        nat.check(nat.lib().vad_a2_loss_grads(p.h, nat.ptr(p.d_s), nat.ptr(p.d_adj), self.stream()))
        return p.d_s.clone(), p.d_adj.clone()

    def backward(self, d_s=None, d_adj=None, d_f=None):
        nat.check(nat.lib().vad_a2_backward(self.cur.h, nat.ptr(d_s) if d_s is not None else None,
                                            nat.ptr(d_adj) if d_adj is not None else None,
                                            nat.ptr(d_f) if d_f is not None else None, self.stream()))

    def optimizer_step(self, lr, weight_decay, max_norm, betas=(0.9, 0.999), eps=1e-8):
        nat.check(nat.lib().vad_a2_optimizer_step(self.cur.h, ctypes.c_float(lr), ctypes.c_float(betas[0]),
                                                  ctypes.c_float(betas[1]), ctypes.c_float(eps),
                                                  ctypes.c_float(weight_decay), ctypes.c_float(max_norm),
                                                  self.stream()))


class _ParamGroups:
    """The slice of the torch optimizer surface the reference's driver reads (param_groups[0]['lr']) and writes into
    its checkpoints (a2:438-455: ``optimizer.state_dict()``).  The AdamW moments live in the engine's flat device
    buffers; ``state_dict`` exports them in torch.optim.AdamW's layout (one entry per parameter, named_parameters
    order) so a checkpoint written here loads into the reference's optimizer and vice versa."""

    def __init__(self, lr, weight_decay, model_ref=None):
        self.param_groups = [{"lr": lr, "weight_decay": weight_decay, "betas": (0.9, 0.999), "eps": 1e-8}]
        self._model_ref = model_ref

    def _engine(self):
        m = self._model_ref() if self._model_ref is not None else None
        return getattr(m, "_engine", None)

    def state_dict(self):
        g = dict(self.param_groups[0])
        e = self._engine()
        n = len(list(self._model_ref().parameters())) if self._model_ref is not None else 0
        state = {}
        if e is not None:
            steps = e.steps.cpu().tolist()
            for i, (_, o, k) in enumerate(e.slots):
                if steps[i] > 0:
                    shape = e.param_views[i].shape
                    state[i] = {"step": torch.tensor(float(steps[i])),
                                "exp_avg": e.exp_avg[o:o + k].view(shape).detach().cpu().clone(),
                                "exp_avg_sq": e.exp_avg_sq[o:o + k].view(shape).detach().cpu().clone()}
        g.update(amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                 params=list(range(n)))
        return {"state": state, "param_groups": [g]}

    def load_state_dict(self, sd):
        g = sd["param_groups"][0]
        for k in ("lr", "weight_decay", "betas", "eps"):
            if k in g:
                self.param_groups[0][k] = tuple(g[k]) if k == "betas" else float(g[k])
        self._pending = sd.get("state", {})
        e = self._engine()
        if e is not None:
            self.push_state(e)

    def push_state(self, e):
        """Copy loaded moments into the engine's device buffers (called once the engine exists)."""
        st = getattr(self, "_pending", None)
        if not st:
            return
        steps = [0] * len(e.slots)
        with torch.no_grad():
            for i, (_, o, k) in enumerate(e.slots):
                s = st.get(i, st.get(str(i)))
                if s is None:
                    continue
                e.exp_avg[o:o + k].copy_(s["exp_avg"].reshape(-1).to(e.exp_avg))
                e.exp_avg_sq[o:o + k].copy_(s["exp_avg_sq"].reshape(-1).to(e.exp_avg_sq))
                steps[i] = int(float(s["step"]))
            e.steps.copy_(torch.tensor(steps, dtype=torch.int32))
        self._pending = None


class _Plateau:
    """ReduceLROnPlateau(mode='min', factor=0.5, patience=5) semantics (torch defaults: rel threshold 1e-4)."""

    def __init__(self, opt, factor=0.5, patience=5, threshold=1e-4, min_lr=0.0, eps=1e-8):
        self.opt, self.factor, self.patience, self.threshold, self.min_lr, self.eps = (
            opt, factor, patience, threshold, min_lr, eps)
        self.best, self.bad = float("inf"), 0

    def state_dict(self):
        return {"factor": self.factor, "patience": self.patience, "threshold": self.threshold,
                "min_lrs": [self.min_lr], "eps": self.eps, "best": self.best, "num_bad_epochs": self.bad,
                "mode": "min", "threshold_mode": "rel", "cooldown": 0, "cooldown_counter": 0}

    def load_state_dict(self, sd):
        self.factor, self.patience = float(sd["factor"]), int(sd["patience"])
        self.threshold, self.eps = float(sd["threshold"]), float(sd["eps"])
        self.min_lr = float(sd.get("min_lrs", [0.0])[0])
        self.best, self.bad = float(sd["best"]), int(sd["num_bad_epochs"])

    def step(self, metric):
        if metric < self.best * (1 - self.threshold):
            self.best, self.bad = metric, 0
        else:
            self.bad += 1
        if self.bad > self.patience:
            for g in self.opt.param_groups:
                new = max(g["lr"] * self.factor, self.min_lr)
                if g["lr"] - new > self.eps:
                    g["lr"] = new
            self.bad = 0


LOSS_KEYS = ("anomaly_loss", "acyclicity_loss", "sparsity_loss", "consistency_loss", "structure_loss", "edge_count",
             "sparsity_ratio")


def _check_batch(B):
    """A single-clip batch fails in the reference: ``anomaly_scores.squeeze()`` is 0-d while the pseudo-targets are
    (1,), and ``F.binary_cross_entropy`` raises (a2:139-147; reproduced by running the reference on B=1)."""
    if B == 1:
        raise ValueError("Using a target size (torch.Size([1])) that is different to the input size "
                         "(torch.Size([])) is deprecated. Please ensure they have the same size.")


class ImprovedMiniCausalVAD:
    """a2:107-297 on the HIP plan: model / optimizer / scheduler attributes, compute_improved_loss,
    train_epoch_improved, evaluate_improved."""

    def __init__(self, device="cuda"):
        self.device = device
        self.model = CausalAnomalyDetector().to(device)
        self.optimizer = _ParamGroups(lr=0.0005, weight_decay=0.001, model_ref=lambda: self.model)
        self.anomaly_weight, self.causal_weight, self.sparsity_weight, self.consistency_weight = 1.0, 0.01, 0.001, 0.01
        self.scheduler = _Plateau(self.optimizer, factor=0.5, patience=5)
        self.seed = 1234
        self.global_step = 0
        self.clip0 = 0

    def compute_improved_loss(self, anomaly_scores, causal_adj, targets, features):
        """Loss of the model's last forward (the labels are ignored: pseudo-labels, a2:139-141).  Returns
        (total loss tensor with autograd into the model's backward, components dict)."""
        _check_batch(anomaly_scores.shape[0])
        e = self.model._engine
        seed, step, clip0 = e.last_keys
        total = _A2LossFunction.apply(anomaly_scores, causal_adj, e, seed, step, clip0)
        vals = e.losses.cpu().tolist()
        return total, dict(zip(LOSS_KEYS, vals[1:8]))

    def train_step(self, videos, labels):
        """One a2:218-245 iteration fused on device (forward + loss + backward + clip + AdamW)."""
        _check_batch(videos.shape[0])
        videos = videos.to(self.device, dtype=torch.float32).contiguous()
        self.model.train()
        e = self.model.engine(videos)
        self.optimizer.push_state(e)
        g = self.optimizer.param_groups[0]
        # The reference reads the loss after the forward and skips the backward and the step on NaN (a2:230-232).
        # Here the forward's copy kernel also writes the losses into pinned host memory (plan option host_losses),
        # the backward and the optimizer step are queued at once -- the optimizer kernels skip the update on device
        # when the loss is NaN (status word losses[9]) and the backward's grads are overwritten by the next one --
        # and the host waits for the forward only, so the device never idles on the host round trip.
        if getattr(self, "_loss_host", None) is None:
            self._loss_host = torch.zeros(10, dtype=torch.float32).pin_memory()
            self._loss_ev = torch.cuda.Event()
        e.set_host_losses(self._loss_host)
        e.forward(videos, True, self.seed, self.global_step, self.clip0, with_loss=True, borrow_input=True)
        self._loss_ev.record()
        e.backward()
        e.optimizer_step(g["lr"], g["weight_decay"], max_norm=0.5)
        self._loss_ev.synchronize()
        vals = self._loss_host.tolist()
        comps = dict(zip(LOSS_KEYS, vals[1:8]))
        stepped = not np.isnan(vals[0])
        self.global_step += 1
        self.clip0 += videos.shape[0]
        return vals[0], comps, stepped

    def train_epoch_improved(self, dataloader):
        total_loss = 0.0
        comps_sum = {k: 0.0 for k in LOSS_KEYS}
        for batch_idx, (videos, labels) in enumerate(dataloader):
            loss, comps, stepped = self.train_step(videos, labels)
            if not stepped:
                print(f"NaN loss detected at batch {batch_idx}, skipping...")
                continue
            total_loss += loss
            for k, v in comps.items():
                comps_sum[k] += v
        n = len(dataloader)
        avg = total_loss / n
        self.scheduler.step(avg)
        return avg, {k: v / n for k, v in comps_sum.items()}

    def evaluate_improved(self, dataloader):
        self.model.eval()
        preds, graphs = [], []
        with torch.no_grad():
            for videos, _ in dataloader:
                videos = videos.to(self.device, dtype=torch.float32).contiguous()
                s, adj, f = self.model(videos)
                preds.extend(s.squeeze().cpu().numpy().reshape(-1).tolist())
                graphs.append(adj.cpu().numpy())
        preds = np.array(preds, dtype=np.float32)
        graphs = np.vstack(graphs)
        e = np.sum(graphs > 0.1, axis=(1, 2))
        metrics = {"mean_score": float(np.mean(preds)), "std_score": float(np.std(preds)),
                   "min_score": float(np.min(preds)), "max_score": float(np.max(preds)),
                   "score_range": float(np.max(preds) - np.min(preds)), "avg_edges": float(np.mean(e)),
                   "avg_sparsity": float(np.mean(e / 256)),
                   "unique_graphs": len(np.unique(graphs.reshape(len(graphs), -1), axis=0))}
        return preds, graphs, metrics

    def save_checkpoint(self, path, **extra):
        """The a2:438-455 checkpoint dict: model / optimizer (/ scheduler) state plus caller extras (epoch, ...)."""
        ck = {"model_state_dict": self.model.state_dict(), "optimizer_state_dict": self.optimizer.state_dict(),
              "scheduler_state_dict": self.scheduler.state_dict()}
        ck.update(extra)
        torch.save(ck, str(path))

    def load_checkpoint(self, path):
        """Load an a2-format checkpoint (incl. the shipped best_improved_model.pth) or a bare state_dict.  Only
        tensors and plain containers are read (weights_only=True)."""
        ck = torch.load(str(path), map_location="cpu", weights_only=True)
        sd = ck.get("model_state_dict", ck) if isinstance(ck, dict) else ck
        self.model.load_state_dict(sd)
        if isinstance(ck, dict) and "optimizer_state_dict" in ck:
            self.optimizer.load_state_dict(ck["optimizer_state_dict"])
        if isinstance(ck, dict) and "scheduler_state_dict" in ck:
            self.scheduler.load_state_dict(ck["scheduler_state_dict"])
        return ck


class MiniCausalVAD(ImprovedMiniCausalVAD):
    """The ``MiniCausalVAD`` surface avenue_training_script1.py drives (a1:19,104,141,160,180-181,187,210): ``.model``
    (whose forward returns the (scores, adj, features) 3-tuple, a1:51), ``.device``, ``.optimizer.param_groups``
    (a1:107-108), ``train_epoch(loader) -> (loss, components)`` with the anomaly/acyclicity/sparsity/consistency
    keys (a1:141-154), ``evaluate(loader) -> (predictions, labels, causal_graphs)`` (a1:160,187) and
    ``save_model/load_model(path)`` (a1:180-181,205,210).  The module a1 imports it from (``minicausal_vad``,
    a1:20) is not in the reference repo, so this restates it on the a2 model and loss it shares its 16x16 causal
    graph and loss keys with; the default lr 1e-3 is the one a1:107 treats as the constructor's.  Semantics beyond
    a1's call sites are parity unpinned."""

    def __init__(self, device="cuda", learning_rate=0.001):
        super().__init__(device)
        self.optimizer.param_groups[0]["lr"] = learning_rate

    def train_epoch(self, dataloader):
        return self.train_epoch_improved(dataloader)

    def evaluate(self, dataloader):
        self.model.eval()
        preds, labels, graphs = [], [], []
        with torch.no_grad():
            for videos, y in dataloader:
                videos = videos.to(self.device, dtype=torch.float32).contiguous()
                s, adj, _ = self.model(videos)
                preds.append(s.reshape(-1).cpu().numpy())
                labels.append(np.asarray(torch.as_tensor(y).reshape(-1).cpu().numpy(), dtype=np.float32))
                graphs.append(adj.cpu().numpy())
        return np.concatenate(preds), np.concatenate(labels), np.concatenate(graphs)

    def save_model(self, path):
        self.save_checkpoint(path, global_step=self.global_step)

    def load_model(self, path):
        ck = self.load_checkpoint(path)
        if isinstance(ck, dict) and "global_step" in ck:
            self.global_step = int(ck["global_step"])
