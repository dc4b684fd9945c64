"""What FlatEngine (vad_amd/_flat.py) promises for each of the five models: the module's parameters and running
statistics alias the flat buffers at the library's offsets, the BatchNorm counters the module shows are the device's,
a second shape adds a plan and moves nothing, load_state_dict writes through the views, and each model keeps its
rebinding mode (``p.data = view`` for cad and ae, new nn.Parameter objects for mc, a2 and bbox: pinned on purpose, so
that unifying them has to change this test).

Each case is the smallest shape the model's GPU tests already run, and runs two forwards.  The counters move by one
per BatchNorm call: once per forward for cad and mc, and T times for cad1's autoencoder, which applies its encoder and
decoder frame by frame (cad1:221-260) -- `nbt_step` below.
"""
import pytest
import torch

from oracle import cad_oracle as co

pytestmark = pytest.mark.gpu


def _cad():
    from vad_amd.cad import CausalAnomalyDetector
    m = CausalAnomalyDetector().cuda()

    def run(B):
        x = co.synth_clips(0, 0, 0, B, 1, 64, 64).cuda()
        m.engine().forward(x, True, 0, 0, 0, co.synth_labels(0, B).cuda())

    return m, run, lambda: m.engine(), True, 1


def _module_case(make, shape, same_objects, nbt_step, train=True):
    m = make().cuda()
    m.train(train)

    def run(B):
        with torch.no_grad():
            m(torch.rand(B, *shape, device="cuda"))

    return m, run, (lambda: m.engine()) if same_objects else (lambda: m._engine), same_objects, nbt_step


def _mc():
    from vad_amd.mc import SimpleVideoAnomalyDetector
    return _module_case(SimpleVideoAnomalyDetector, (1, 8, 32, 32), False, 1)


def _a2():
    from vad_amd.a2 import CausalAnomalyDetector
    return _module_case(CausalAnomalyDetector, (3, 8, 64, 64), False, 0)


def _ae():
    from vad_amd.ae import VideoAutoEncoder
    return _module_case(VideoAutoEncoder, (8, 1, 64, 64), True, 8)


def _bbox():
    from vad_amd.bbox import CausalAnomalyDetector
    return _module_case(CausalAnomalyDetector, (3, 8, 64, 64), False, 0, train=False)


CASES = {"cad": (_cad, 2), "mc": (_mc, 4), "a2": (_a2, 4), "ae": (_ae, 4), "bbox": (_bbox, 3)}


def _pointers(m):
    return [t.data_ptr() for t in list(m.parameters()) + list(m.buffers())]


@pytest.mark.parametrize("name", list(CASES))
def test_module_aliases_flat_buffers(name):
    make, B = CASES[name]
    torch.manual_seed(0)
    m, run, engine, same_objects, nbt_step = make()
    before = list(m.parameters())
    nbt0 = {k: int(v) for k, v in m.state_dict().items() if k.endswith("num_batches_tracked")}
    assert bool(nbt0) == (nbt_step > 0)
    run(B)
    e = engine()
    after = list(m.parameters())
    if same_objects:
        assert all(a is b for a, b in zip(before, after))
    else:
        assert not any(a is b for a, b in zip(before, after))
    named = dict(m.named_parameters())
    assert list(named) == [k for k, _, _ in e.slots]
    for k, off, n in e.slots:
        assert named[k].data_ptr() == e.params.data_ptr() + 4 * off and named[k].numel() == n, k
    bufs = dict(m.named_buffers())
    assert [k for k, _, _ in e.buf_slots] == [k for k in bufs if "running_" in k]
    for k, off, n in e.buf_slots:
        assert bufs[k].data_ptr() == e.bufs.data_ptr() + 4 * off and bufs[k].numel() == n, k
    torch.cuda.synchronize()
    for k, v0 in nbt0.items():
        assert int(bufs[k]) == v0 + nbt_step, k
    base, ptrs = e.params.data_ptr(), _pointers(m)
    assert len(e.plans) == 1
    run(B + 1)
    assert engine() is e and len(e.plans) == 2 and e.params.data_ptr() == base and _pointers(m) == ptrs
    m.load_state_dict(m.state_dict())
    assert engine() is e and e.params.data_ptr() == base and _pointers(m) == ptrs
