"""The fused optimizer keeps the cad plan's weight images current (plan option opt_images, knob cad_opt_images).

The images -- the conv relayouts wf / wd (plain or the stride-2 class form, the pre-split bf16 planes, the bf16
copies) and the detector's transposed layers wt -- are written by one store routine (csrc/weight_images.h), called by
the relayout kernels and by adamw_kernel, and a forward relayouts only when the images are not known to hold the
parameters.  Everything here is bit-exact: the knob-off path is the plain optimizer plus a relayout before every
forward.  Shapes: B=2, T=4 at 64 x 64 (the small golden cases' frame) and at the ragged 37 x 45."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import cad_oracle as co
from tests.golden.cases import FORCED_A
from tests.golden_util import make_cad_model, read_debug, read_debug_len

pytestmark = pytest.mark.gpu
B, T = 2, 4
FRAMES = [(64, 64), (37, 45)]
OUT_KEYS = ("final", "probs", "causal", "kl", "z", "adj", "nmax", "boxes", "counts")


@contextlib.contextmanager
def _opt_images(on):
    from vad_amd import _native as nat
    nat.check(nat.lib().vad_set_tuning(b"cad_opt_images", int(on)))
    try:
        yield
    finally:
        nat.check(nat.lib().vad_set_tuning(b"cad_opt_images", 1))


def _model(forced, frozen=True, seed=1):
    from vad_amd.train import apply_memory_efficient_training
    m = make_cad_model(dict(seed=seed, forced=FORCED_A if forced else None))
    if frozen:
        with contextlib.redirect_stdout(io.StringIO()):
            apply_memory_efficient_training(m)
    return m.cuda()


def _data(H, W, seed=1):
    return co.synth_clips(seed, 0, 0, B, T, H, W).cuda(), co.synth_labels(0, B).cuda()


def _set_option(pl, key, v):
    from vad_amd import _native as nat
    nat.check(nat.lib().vad_cad_set_option(pl.h, key, v))


def _images(pl):
    """Every weight image buffer of the plan, whole, as raw 32-bit words."""
    out = {}
    for l in range(8):
        out[f"wf{l}"] = read_debug(pl, "wf", l, dtype=np.uint32)
        out[f"wd{l}"] = read_debug(pl, "wd", l, dtype=np.uint32)
    for i in range(1, 5):
        out[f"wt{i}"] = read_debug(pl, "wt", i, dtype=np.uint32)
    return out


def _eval(eng, x):
    o = eng.forward(x, False, 0, 0, 0)
    torch.cuda.synchronize()
    return {k: o[k].clone() for k in OUT_KEYS}


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("H,W", FRAMES, ids=["64x64", "37x45"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_optimizer_images_equal_relayout(dtype, H, W):
    """After a trainer step the images the optimizer wrote equal, byte for byte, what the relayout kernels make of the
    same parameters (forced-detection regime: the detector's slots are active, so wt is really rewritten)."""
    from vad_amd.train import CadTrainer
    m = _model(forced=True)
    tr = CadTrainer(m, lr=3e-4, seed=0, compute_dtype=dtype)
    x, y = _data(H, W)
    tr.step(x, y)
    torch.cuda.synchronize()
    pl = tr.eng.plan(B, T, H, W)
    assert read_debug_len(pl, "images_fresh") == 1
    first = _images(pl)
    tr.step(x, y)
    torch.cuda.synchronize()
    assert float(tr.eng.grads[tr.eng.param_floats]) > 0  # the detector had a grad
    assert read_debug_len(pl, "images_fresh") == 1
    mine = _images(pl)
    for k in ("wf0", "wd7", "wt1", "wt4"):  # (the second step's optimizer did write them)
        assert not np.array_equal(mine[k], first[k]), k
    _set_option(pl, b"images_fresh", 0)
    tr.eng.forward(x, False, 0, 0, 0)
    torch.cuda.synchronize()
    ref = _images(pl)
    for k in ref:
        np.testing.assert_array_equal(mine[k], ref[k], err_msg=k)


def _train_state(on, forced, frozen, H, W, steps=3):
    from vad_amd.train import CadTrainer
    with _opt_images(on):
        m = _model(forced, frozen)
        tr = CadTrainer(m, lr=3e-4, seed=0)
        x, y = _data(H, W)
        losses = [tr.step(x, y).clone() for _ in range(steps)]
        torch.cuda.synchronize()
        e = tr.eng
        return dict(params=e.params.cpu(), exp_avg=e.exp_avg.cpu(), exp_avg_sq=e.exp_avg_sq.cpu(), steps=e.steps.cpu(),
                    bufs=e.bufs.cpu(), nbt=e.nbt.cpu(), losses=torch.stack(losses).cpu())


@pytest.mark.parametrize("H,W", FRAMES, ids=["64x64", "37x45"])
@pytest.mark.parametrize("frozen", [True, False], ids=["stem-frozen", "stem-trains"])
@pytest.mark.parametrize("forced", [False, True], ids=["fallback", "forced"])
def test_steps_equal_option_off(forced, frozen, H, W):
    """Three CadTrainer steps with the optimizer writing the images equal three steps of the plain optimizer with a
    relayout per forward: parameters, both moment buffers, step counters, losses and BN buffers, bit for bit."""
    on = _train_state(1, forced, frozen, H, W)
    off = _train_state(0, forced, frozen, H, W)
    for k in on:
        assert torch.equal(on[k], off[k]), k


def _dp_worker(rank, world, port, on, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from tests.dp_util import make_batches
        from vad_amd.train import CadTrainer
        with _opt_images(on):
            m = _model(forced=True)
            x, y = make_batches(world, B=B, T=T, H=64, W=64)[rank]
            tr = CadTrainer(m, lr=3e-4, seed=0)
            for _ in range(3):
                tr.step(x.cuda(), y.cuda())
            torch.cuda.synchronize()
            if rank == 0:
                e = tr.eng
                torch.save({"params": e.params.cpu(), "exp_avg": e.exp_avg.cpu(), "exp_avg_sq": e.exp_avg_sq.cpu(),
                            "steps": e.steps.cpu(), "bufs": e.bufs.cpu()}, out_path)
    finally:
        dist.destroy_process_group()


def test_steps_equal_option_off_two_ranks(tmp_path):
    """The same over two gloo ranks on cuda:0 (the stage 2 / stage 1 backward with its bucketed all-reduces; the
    trainer's parameter broadcast is a write behind the plan's back that the engine must see)."""
    from tests.test_dp import _free_port
    res = {}
    for on in (1, 0):
        out = str(tmp_path / f"on{on}.pt")
        mp.spawn(_dp_worker, args=(2, _free_port(), on, out), nprocs=2, join=True)
        res[on] = torch.load(out, weights_only=True)
    for k in res[1]:
        assert torch.equal(res[1][k], res[0][k]), k


@pytest.mark.parametrize("write", ["load_state_dict", "inplace_mul"])
def test_foreign_writes_are_seen(write):
    """Parameters written from torch between two steps (behind the plan's back) invalidate the images: the next
    forward equals that of a fresh engine built from the same state, and differs from the forward before the write
    (so stale images could not pass)."""
    from vad_amd.train import CadTrainer
    m = _model(forced=True)
    tr = CadTrainer(m, lr=3e-4, seed=0)
    x, y = _data(64, 64)
    tr.step(x, y)
    before = _eval(tr.eng, x)
    names = ("backbone.layer2.0.weight", "detector.detector_net.3.weight")
    if write == "load_state_dict":
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        for n in names:
            sd[n] *= 1.25
        m.load_state_dict(sd)
    else:
        ps = dict(m.named_parameters())
        with torch.no_grad():
            for n in names:
                ps[n].mul_(1.25)
    after = _eval(tr.eng, x)
    fresh = _model(forced=True, seed=7)
    fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
    want = _eval(fresh.engine(), x)
    for k in OUT_KEYS:
        assert torch.equal(after[k], want[k]), k
    assert not _same(after, before)
    tr.step(x, y)  # and training goes on from the written parameters
    torch.cuda.synchronize()
    assert read_debug_len(tr.eng.plan(B, T, 64, 64), "images_fresh") == 1


def _two_plans(on):
    from vad_amd.train import CadTrainer
    with _opt_images(on):
        m = _model(forced=True)
        tr = CadTrainer(m, lr=3e-4, seed=0)
        xa, ya = _data(64, 64)
        xb, _ = _data(37, 45, seed=2)
        out = []
        out.append({"losses": tr.step(xa, ya).clone()})
        out.append(_eval(tr.eng, xb))
        out.append({"losses": tr.step(xa, ya).clone()})
        out.append(_eval(tr.eng, xb))  # (plan B's images are stale now: plan A's optimizer stepped the parameters)
        out.append(_eval(tr.eng, xa))
        out.append({"losses": tr.step(xa, ya).clone()})
        torch.cuda.synchronize()
        out.append({"params": tr.eng.params.clone(), "bufs": tr.eng.bufs.clone()})
        return out


def test_two_plans_share_parameters_not_images():
    """Train on shape A, eval on shape B, train on A again ...: each result equals the option-off run."""
    on, off = _two_plans(1), _two_plans(0)
    for i, (a, b) in enumerate(zip(on, off)):
        for k in a:
            assert torch.equal(a[k], b[k]), (i, k)
    assert not _same(on[1], on[3])  # (the step between the two B forwards moved their outputs)


def test_repeated_eval_forwards_skip_relayout():
    """The second of two eval forwards on unchanged weights launches no relayout (no "prep" record among the plan's
    profile labels) and returns the same outputs."""
    m = _model(forced=True)
    eng = m.engine()
    x, _ = _data(64, 64)
    eng.forward(x, False, 0, 0, 0)  # (builds the plan)
    pl = eng.plan(B, T, 64, 64)
    _set_option(pl, b"images_fresh", 0)
    eng.profile(True)
    first = _eval(eng, x)
    labels1 = eng.profile_read()
    eng.profile(True)
    second = _eval(eng, x)
    labels2 = eng.profile_read()
    eng.profile(False)
    assert labels1["prep"][1] == 2  # the conv relayout and the detector transposes
    assert "prep" not in labels2 and "conv_fwd/L0" in labels2
    assert _same(first, second)
