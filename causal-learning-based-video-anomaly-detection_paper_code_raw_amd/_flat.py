"""FlatEngine / FlatPlan: what the five engines (cad, mc, a2, bbox, ae) share.

The library lays every model out the same way (csrc/plan_util.h FlatLayout): parameters in named_parameters()
order and BatchNorm running statistics in state_dict order, each slot at a 256-float-aligned offset of one flat fp32
buffer.  FlatEngine reads that table through the model's C prefix, allocates the flat buffers on the model's HIP
device and points the module at views of them, so state_dict / load_state_dict keep working:
  * params, grads (+ grad_tail floats the model's kernels use for flags), bufs (running_mean / running_var), nbt (the
    num_batches_tracked counters, int64), exp_avg / exp_avg_sq / steps (Adam state);
  * one FlatPlan (C plan + 256-B aligned workspace) per input shape, all bound to the same buffers.
Two things differ between the models for historical reasons and are constructor arguments, not code:
  * replace_params: False rebinds with ``p.data = view`` (the Parameter objects survive; cad, ae), True installs new
    nn.Parameter objects over the views (mc, a2, bbox);
  * opt_state: "lazy" allocates the Adam state on the first optimizer step and rebinds the plans (cad, ae), "eager"
    with the engine (mc, a2), None never (bbox).
Everything derived from the tables is computed once here: nothing below runs per step.
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn

from . import _native as nat

_NAME_MISMATCH = (RuntimeError, "model parameters do not match the libvadhip slot table")


def _set_buffer(model, dotted, tensor):
    mod_name, _, attr = dotted.rpartition(".")
    model.get_submodule(mod_name)._buffers[attr] = tensor


class FlatPlan:
    """One C plan + workspace per input shape (the engine's cache key), bound to the engine's flat buffers."""

    def __init__(self, e: "FlatEngine", *key):
        self.h = ctypes.c_void_p()
        self._destroy = e.fn("destroy")
        nat.check(e.fn("create")(*self.create_args(*key), ctypes.byref(self.h)))
        self.configure(e, *key)  # (options the workspace size depends on go in before the size query)
        self.ws = torch.empty(int(e.fn("workspace_bytes")(self.h)) + 256, dtype=torch.uint8, device=e.device)
        self.bind(e)

    @staticmethod
    def create_args(*key):
        return key

    def configure(self, e, *key):
        pass

    def bind(self, e):
        base = (self.ws.data_ptr() + 255) // 256 * 256
        nat.check(e.fn("bind")(self.h, ctypes.c_void_p(base), *[nat.ptr(getattr(e, k)) for k in e.bind_names]))

    def __del__(self):
        try:
            if self.h:
                self._destroy(self.h)
        except Exception:
            pass


class FlatEngine:
    PLAN = FlatPlan

    def __init__(self, model, device, prefix, *, replace_params, opt_state, bind_names, grad_tail=0,
                 name_mismatch=_NAME_MISMATCH):
        self.model, self.device, self.prefix = model, device, prefix
        self.bind_names, self.opt_state = bind_names, opt_state
        self.slots, self.slot_group, self.param_floats, self.buf_slots, buf_floats = self._read_tables(model)
        self.slot_names = [s[0] for s in self.slots]
        self.slot_offset = [s[1] for s in self.slots]
        self.slot_numel = [s[2] for s in self.slots]
        named = list(model.named_parameters())
        if [k for k, _ in named] != self.slot_names:
            raise name_mismatch[0](name_mismatch[1])
        for (k, p), nel in zip(named, self.slot_numel):
            if p.numel() != nel:
                raise RuntimeError(f"parameter {k}: {p.numel()} elements, library expects {nel}")
        f = dict(dtype=torch.float32, device=device)
        self.params = torch.zeros(self.param_floats, **f)
        self.grads = torch.zeros(self.param_floats + grad_tail, **f)
        self.param_views = [self.params[o:o + n].view_as(p) for (_, o, n), (_, p) in zip(self.slots, named)]
        self._grad_views = [self.grads[o:o + n].view_as(p) for (_, o, n), (_, p) in zip(self.slots, named)]
        self.exp_avg = self.exp_avg_sq = self.steps = self.bufs = self.nbt = None
        with torch.no_grad():
            for (k, p), view in zip(named, self.param_views):
                view.copy_(p.detach())
                if replace_params:
                    mod_name, _, attr = k.rpartition(".")
                    setattr(model.get_submodule(mod_name), attr, nn.Parameter(view, requires_grad=p.requires_grad))
                else:
                    p.data = view
            if self.buf_slots:
                named_bufs = dict(model.named_buffers())
                self.bufs = torch.zeros(buf_floats, **f)
                for k, o, n in self.buf_slots:
                    view = self.bufs[o:o + n].view_as(named_bufs[k])
                    view.copy_(named_bufs[k])
                    _set_buffer(model, k, view)
                nbt_names = [k for k in named_bufs if k.endswith("num_batches_tracked")]
                self.nbt = torch.zeros(len(nbt_names), dtype=torch.int64, device=device)
                for i, k in enumerate(nbt_names):
                    self.nbt[i].copy_(named_bufs[k].reshape(()))
                    _set_buffer(model, k, self.nbt[i])
        self.plans = {}
        self.cur = None
        if opt_state == "eager":
            self.init_optimizer_state()

    def fn(self, name):
        return getattr(nat.lib(), f"vad_{self.prefix}_{name}")

    def _read_tables(self, model):
        """-> (slots, groups, param_floats, buf_slots, buf_floats); slots as (name, offset, numel) tuples."""
        L, pre, probe = nat.lib(), (), None
        if self.prefix == "mc":
            # mc's accessors take a plan (its table depends on the model's input channels, on nothing else of the
            # shape): read them off a throw-away one
            probe = ctypes.c_void_p()
            nat.check(L.vad_mc_create(1, model.features[0].in_channels, 8, 8, 8, ctypes.byref(probe)))
            pre = (probe,)

        def table(kind, total):
            if not hasattr(L, f"vad_{self.prefix}_num_{kind}s"):
                return [], 0
            name, off, numel = (self.fn(f"{kind}_{a}") for a in ("name", "offset", "numel"))
            return ([(name(*pre, i).decode(), off(*pre, i), numel(*pre, i))
                     for i in range(self.fn(f"num_{kind}s")(*pre))], self.fn(total)(*pre))

        try:
            slots, nparam = table("slot", "param_floats")
            bufs, nbuf = table("buf", "buf_floats")
            groups = ([self.fn("slot_group")(i) for i in range(len(slots))]
                      if hasattr(L, f"vad_{self.prefix}_slot_group") else None)
        finally:
            if probe is not None:
                L.vad_mc_destroy(probe)
        return slots, groups, nparam, bufs, nbuf

    def init_optimizer_state(self):
        if self.exp_avg is None:
            self.exp_avg = torch.zeros_like(self.params)
            self.exp_avg_sq = torch.zeros_like(self.params)
            self.steps = torch.zeros(len(self.slots), dtype=torch.int32, device=self.device)
            for p in self.plans.values():
                p.bind(self)

    def is_bound(self) -> bool:
        p = next(self.model.parameters())
        return p.data_ptr() == self.params.data_ptr() and p.device == self.device

    def plan(self, *key):
        pl = self.plans.get(key)
        if pl is None:
            pl = self.plans[key] = self.PLAN(self, *key)
        return pl

    def stream(self):
        return nat.stream_of(self.device)

    def grad_clones(self):
        """Per-parameter copies of the flat grads, in named_parameters() order and shape (what autograd is handed)."""
        return [g.clone() for g in self._grad_views]

    def grad_dict(self):
        """{parameter name: its flat slice of grads} (views, not copies)."""
        return {k: self.grads[o:o + n] for k, o, n in self.slots}
