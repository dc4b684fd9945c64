"""C ABI checks that need no GPU: the library loads, exports every function include/vad.h declares and is bound with
the signatures the header declares, its slot table matches the drop-in module's parameters, and errors come back as
codes + text."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "vad.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(vad_\w+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from vad_amd import _native
    L = _native.lib()
    names = _declared()
    assert len(names) >= 20
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing
    assert L.vad_abi_version() == 1


_P, _I, _I64, _U64, _U32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint32
_F, _D, _S = ctypes.c_float, ctypes.c_double, ctypes.c_char_p

_HEADER_CASES = """
/* a header in the small: every form include/vad.h holds */
#ifndef X_H_
#define X_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define VAD_ABI_VERSION 1
int vad_abi_version(void);
const char* vad_last_error(void);
typedef struct vad_x_plan vad_x_plan;
int vad_x_create(int B, int T, vad_x_plan** out);
void vad_x_destroy(vad_x_plan* plan);
int64_t vad_x_workspace_bytes(const vad_x_plan* p);   /* bytes (not floats) */
/* broken over three lines, a comment with ( brackets ) and a , between two parameters */
int vad_x_forward(vad_x_plan* plan, const float* x, int training, uint64_t seed,
                  uint32_t stream_id, /* keyed (seed, step) draws */ int64_t clip0, float scale, double drop_p,
                  const int32_t* flags, const float* const* W, void* stream);
typedef int (*vad_bn_sync_fn)(void* user, int bn_layer, int phase, int64_t n, void* stream);
int vad_x_set_bn_sync(vad_x_plan* plan, vad_bn_sync_fn fn, void* user, int world);
int vad_x_set_option(vad_x_plan* plan, const char* key, int64_t value);
int vad_x_profile_read(vad_x_plan* plan, char* labels, double* total_ms, int* counts, int cap);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_header_parser_forms():
    """_parse_header on literal text: every form of declaration and parameter vad.h holds, the lines it skips, and its
    refusal to guess."""
    from vad_amd import _native
    parse = _native._parse_header
    assert parse(_HEADER_CASES) == {
        "vad_abi_version": (_I, []),
        "vad_last_error": (_S, []),
        "vad_x_create": (_I, [_I, _I, _P]),
        "vad_x_destroy": (None, [_P]),
        "vad_x_workspace_bytes": (_I64, [_P]),
        "vad_x_forward": (_I, [_P, _P, _I, _U64, _U32, _I64, _F, _D, _P, _P, _P]),
        "vad_x_set_bn_sync": (_I, [_P, _native.BN_SYNC_FN, _P, _I]),
        "vad_x_set_option": (_I, [_P, _S, _I64]),
        "vad_x_profile_read": (_I, [_P, _P, _P, _P, _I]),
    }
    assert _native.BN_SYNC_FN._restype_ is _I and _native.BN_SYNC_FN._argtypes_ == (_P, _I, _I, _I64, _P)
    for text, words in [("int vad_x_f(int a, size_t n);", ("vad_x_f", "size_t")),          # a scalar not in the table
                        ("int vad_x_g(vad_x_plan plan);", ("vad_x_g", "vad_x_plan")),      # a struct by value
                        ("int vad_x_h(int32_t v, void* stream);", ("vad_x_h", "int32_t")),
                        ("size_t vad_x_i(void);", ("vad_x_i", "size_t")),                  # an unknown return type
                        ("int vad_x_j(int);", ("vad_x_j", "int")),                         # no parameter name
                        ("int vad_x_k();", ("vad_x_k",)),
                        ("int vad_x_l(void); int vad_x_l(int a);", ("vad_x_l",)),          # declared twice
                        ("int vad_x_m(int a) { return a; }", ("vad_x_m",)),                # not a declaration
                        ("struct vad_x_plan { int a; };", ("struct",))]:
        with pytest.raises(ValueError) as e:
            parse(text)
        assert all(w in str(e.value) for w in words), (text, str(e.value))


# typed from include/vad.h by hand, so that the parser cannot pass by agreeing with itself
_PINNED = {
    "vad_last_error": (_S, []),
    "vad_cad_destroy": (None, [_P]),
    "vad_cad_slot_offset": (_I64, [_I]),
    "vad_cad_forward": (_I, [_P, _P, _I, _U64, _U64, _I64] + [_P] * 13),
    "vad_cad_windows_forward_group": (_I, [_P, _P, _I64, _I, _I, _P, _I, _P, _U64, _U64] + [_P] * 8),
    "vad_cad_optimizer_step": (_I, [_P] + [_F] * 7 + [_P, _P]),
    "vad_cad_set_option": (_I, [_P, _S, _I64]),
    "vad_cad_profile_read": (_I, [_P, _P, _P, _P, _I]),
    "vad_dense_forward_ex": (_I, [_P, _I, _I, _P, _P, _I, _P, _I, _D, _U64, _U32, _U64, _I64, _I, _P, _I64, _P]),
    "vad_ae_bind": (_I, [_P] * 11),
    "vad_ingest_u8_color": (_I, [_P, _I64, _I, _I, _I64, _I64, _I, _I, _I, _I, _I, _P, _P]),
    "vad_head_backward": (_I, [_P, _I, _I, _P, _I, _U64, _U64, _I64] + [_P] * 16 + [_I64, _P]),
}


def test_signatures_come_from_the_header():
    """Every function vad.h declares has its entry in _SIGS, the loaded library carries exactly those types, and the
    entries pinned above are what the header says."""
    from vad_amd import _native
    L = _native.lib()
    names = _declared()
    assert sorted(_native._SIGS) == names
    for name in names:
        res, args = _native._SIGS[name]
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    for name, sig in _PINNED.items():
        assert _native._SIGS[name] == sig, name
    assert _native._SIGS["vad_cad_set_bn_sync"] == (_I, [_P, _native.BN_SYNC_FN, _P, _I])


# the tuning keys the test suite sets: retiring one of them would strand a test
_KEYS_TESTS_SET = [
    "conv_patch", "conv_patch_persist", "conv_split", "conv_wgrad_patch", "conv_wgrad_split", "conv_wgrad_split_s2",
    "conv_wgrad_tr", "conv_wgrad_tr_pft", "conv_dgrad_s2_x3", "conv_dgrad_s2_w3", "conv_bf16", "act_bf16", "stem_fused",
    "mlp_tail_rb", "mlp_tail_wide", "cad_stem_early", "cad_dir_affine", "cad_opt_images",
    "conv3d_direct", "maxpool3d_bwd_win", "bbox_im2col", "ae_direct", "ae_wgrad_stream", "conv4_cls_batch_min",
    "a2_direct", "a2_head_clip",
]


def test_tuning_table():
    """The knob table (csrc/tuning.h) through vad_tuning_name / vad_get_tuning / vad_set_tuning: unique keys, every key
    reads and writes its own variable, unknown keys are refused by both entry points."""
    from vad_amd import _native
    L = _native.lib()
    keys = []
    while L.vad_tuning_name(len(keys)) is not None:
        keys.append(L.vad_tuning_name(len(keys)))
    assert L.vad_tuning_name(len(keys) + 1) is None and L.vad_tuning_name(-1) is None
    assert len(keys) >= len(_KEYS_TESTS_SET) and len(set(keys)) == len(keys)
    get = lambda k: (_native.check(L.vad_get_tuning(k, ctypes.byref(v))), v.value)[1]
    v = ctypes.c_int()
    entry = {k: get(k) for k in keys}
    try:
        for i, k in enumerate(keys):  # a value of its own per key: two keys on one variable would read back alike
            _native.check(L.vad_set_tuning(k, entry[k] + 100 + i))
        assert {k: get(k) for k in keys} == {k: entry[k] + 100 + i for i, k in enumerate(keys)}
    finally:
        for k in keys:
            L.vad_set_tuning(k, entry[k])
    assert {k: get(k) for k in keys} == entry
    assert L.vad_set_tuning(b"no_such_knob", 1) != 0
    assert b"unknown tuning key no_such_knob" in L.vad_last_error()
    assert L.vad_get_tuning(b"no_such_knob", ctypes.byref(v)) != 0
    assert b"unknown tuning key no_such_knob" in L.vad_last_error()
    missing = [k for k in _KEYS_TESTS_SET if k.encode() not in keys]
    assert not missing, missing


def _cad_model():
    from vad_amd.cad import CausalAnomalyDetector
    return CausalAnomalyDetector()


def _mc_model(C):
    from vad_amd.mc import SimpleVideoAnomalyDetector
    return SimpleVideoAnomalyDetector(input_channels=C)


def _a2_model():
    from vad_amd.a2 import CausalAnomalyDetector
    return CausalAnomalyDetector()


def _bbox_model():
    from vad_amd.bbox import CausalAnomalyDetector
    return CausalAnomalyDetector()


def _ae_model():
    from vad_amd.ae import VideoAutoEncoder
    return VideoAutoEncoder()


# id -> (C prefix, model, has a buffer table, mc's input channels: its accessors take a plan)
_LAYOUTS = {"cad": ("cad", _cad_model, True, None), "mc_c1": ("mc", lambda: _mc_model(1), True, 1),
            "mc_c3": ("mc", lambda: _mc_model(3), True, 3), "a2": ("a2", _a2_model, False, None),
            "bbox": ("bbox", _bbox_model, False, None), "ae": ("ae", _ae_model, True, None)}


@pytest.mark.parametrize("name", list(_LAYOUTS))
def test_slot_table_matches_module(name):
    """Every model's library tables against its module: slots = named_parameters(), buffers = the BN running stats in
    state_dict order, both laid out by the one rule (running sum, each slot rounded up to 256 floats)."""
    from vad_amd import _native
    L = _native.lib()
    pfx, make, has_bufs, C = _LAYOUTS[name]
    torch.manual_seed(0)
    m = make()
    pre = ()
    if C is not None:
        h = ctypes.c_void_p()
        assert L.vad_mc_create(1, C, 4, 8, 8, ctypes.byref(h)) == 0  # the smallest legal shape; runs on the host
        pre = (h,)

    def check(kind, total, want):
        fn = lambda s: getattr(L, f"vad_{pfx}_{s}")  # noqa: E731
        n = fn(f"num_{kind}s")(*pre)
        assert n == len(want)
        off = 0
        for i, (k, numel) in enumerate(want):
            assert fn(f"{kind}_name")(*pre, i).decode() == k
            assert fn(f"{kind}_numel")(*pre, i) == numel
            assert fn(f"{kind}_offset")(*pre, i) == off, k
            off += (numel + 255) // 256 * 256
        assert fn(total)(*pre) == off
        for i in (-1, n):
            assert fn(f"{kind}_name")(*pre, i) is None
            assert fn(f"{kind}_numel")(*pre, i) == -1 and fn(f"{kind}_offset")(*pre, i) == -1

    try:
        named = [(k, p.numel()) for k, p in m.named_parameters()]
        check("slot", "param_floats", named)
        if has_bufs:
            check("buf", "buf_floats", [(k, v.numel()) for k, v in m.state_dict().items() if "running_" in k])
    finally:
        if pre:
            L.vad_mc_destroy(pre[0])
    if name == "cad":
        assert L.vad_cad_slot_group(-1) == -1 and L.vad_cad_slot_group(len(named)) == -1
        groups = {L.vad_cad_slot_name(i).decode(): L.vad_cad_slot_group(i) for i in range(len(named))}
        assert groups["backbone.conv1.weight"] == 0 and groups["structure_learner.structure_params"] == 4
        assert groups["detector.detector_net.0.weight"] == 2 and groups["structure_learner.node_encoder.weight"] == 3
    if name == "ae":
        h = ctypes.c_void_p()
        assert L.vad_ae_create(501, 8, ctypes.byref(h)) != 0  # update_memory writes B rows of the 500-row ring
        assert b"unsupported shape" in L.vad_last_error()


def test_error_codes_and_text():
    from vad_amd import _native
    L = _native.lib()
    h = ctypes.c_void_p()
    rc = L.vad_cad_create(0, 16, 227, 227, ctypes.byref(h))
    assert rc != 0
    assert b"unsupported shape" in L.vad_last_error()


def test_rng_contract_properties():
    keep = rng.dropout_keep(1, rng.S_DET_DROP1, 0, 0, 512, 512, 0.3)
    assert abs(keep.mean() - 0.7) < 0.01
    eps = rng.normal_eps(1, rng.S_EPS, 0, 0, 256, 256)
    assert abs(eps.mean()) < 0.02 and abs(eps.std() - 1) < 0.02
    a = rng.u24(5, 2, 3, np.arange(4), np.arange(7))
    b = rng.u24(5, 2, 3, np.arange(4), np.arange(7))
    assert (a == b).all() and a.max() < (1 << 24)
    assert not (rng.u24(5, 2, 4, np.arange(4), np.arange(7)) == a).all()  # the step changes the draws
    px = rng.pixels_u8(0, 0, 0, 2, 4096)
    assert px.dtype == np.uint8 and px.min() == 0 and px.max() == 255


def test_conv3d_paths_refuse_what_they_do_not_run():
    """vad_conv3d_* name one kernel family; a combination that family does not run is an error with a text that says
    why (never a fall-back to another family).  The checks precede any launch, so no device is needed."""
    from vad_amd import _native
    L = _native.lib()
    fwd = lambda path, Ci, Co, s, layout=1: L.vad_conv3d_forward(
        None, layout, 1, Ci, 4, 8, 8, None, None, Co, s, s, s, path, None, None, 0, None)
    for args, text in [((1, 8, 16, 2), b"path 1 (direct) is stride 1"),
                       ((1, 32, 16, 1), b"needs Ci <= 16"),
                       ((1, 8, 24, 1), b"Co in {8, 16, 32}"),
                       ((2, 16, 32, 1), b"path 2 (conv3s2) is stride 2"),
                       ((2, 3, 16, 2), b"needs Ci % 4 == 0"),
                       ((2, 16, 32, 2, 0), b"reads NDHWC"),
                       ((3, 8, 64, 1), b"needs Ci % 16 == 0"),
                       ((4, 8, 8, 1), b"unknown path"),
                       ((0, 8, 8, 1), b"scratch too small")]:
        assert fwd(*args) != 0
        assert text in L.vad_last_error(), (args, L.vad_last_error())
    assert L.vad_conv3d_dgrad(None, 1, 32, 4, 8, 8, None, 64, 1, 1, 1, 3, None, None, None, 0, None) != 0
    assert b"forward only" in L.vad_last_error()
    assert L.vad_conv3d_dgrad(None, 1, 3, 4, 8, 8, None, 8, 1, 1, 1, 1, None, None, None, 0, None) != 0
    assert b"input gradient needs Ci in {8, 16}" in L.vad_last_error()
    assert L.vad_conv3d_scratch_floats(1, 3, 1, 32, 4, 8, 8, 64, 1, 1, 1) < 0
    assert L.vad_conv3d_scratch_floats(0, 0, 2, 3, 5, 37, 27, 16, 1, 2, 2) >= 2 * 5 * 19 * 14 * 81


def test_dense_and_mlp_entry_points_refuse_before_any_launch():
    """The stand-alone dense / MLP-chain entry points hand their arguments to the launchers, whose host checks precede
    any launch: a refused call returns non-zero with the launcher's text and needs no device."""
    from vad_amd import _native
    L = _native.lib()
    ia = lambda *v: (ctypes.c_int * len(v))(*v)
    none = (ctypes.c_void_p * 8)()
    for nseg in (0, 7):
        assert L.vad_rows_wgrad(4, nseg, none, none, none, none, ia(*[8] * 8), ia(*[8] * 8), None, None) != 0
        assert b"rows_wgrad: bad segment count" in L.vad_last_error()
    assert L.vad_dense_wgrad(None, 17, 5, None, 7, None, None, None, None, 5 * 8 - 1, 256, None) != 0
    assert b"dense_wgrad: scratch too small" in L.vad_last_error()
    fwd = lambda M, K0, N: L.vad_mlp_tail_forward(
        None, M, K0, ia(*N), none, none, ia(1, 1, 1, 1, 0), (ctypes.c_double * 5)(), (ctypes.c_uint32 * 5)(), 0, 0, 0,
        0, none, None, 0, None)
    for K0, N in [(40, (8, 6, 8, 8, 4)),      # a width that is no multiple of 4
                  (40, (12, 8, 8, 8, 4)),     # layer 1's input width no multiple of 8
                  (40, (8, 8, 8, 8, 3)),
                  (40, (1024, 8, 8, 8, 4)),   # wider than the LDS rows
                  (40, (8, 8, 520, 8, 4))]:
        assert fwd(3, K0, N) != 0
        assert b"mlp_tail_fwd: layer shape" in L.vad_last_error(), (N, L.vad_last_error())
    try:
        assert L.vad_set_tuning(b"mlp_tail_rb", 3) == 0
        assert fwd(3, 40, (8, 8, 8, 8, 4)) != 0
        assert b"mlp_tail_fwd: rows per block 2, 4 or 8" in L.vad_last_error()
    finally:
        L.vad_set_tuning(b"mlp_tail_rb", 0)
    # a legal chain gets past those checks and stops at the wrapper's own, still before any launch
    assert fwd(3, 40, (8, 8, 8, 8, 4)) != 0
    assert b"vad_mlp_tail_forward: scratch too small" in L.vad_last_error()
    assert L.vad_mlp_tail_backward(3, None, none, ia(40, 8, 8, 8, 8), ia(8, 8, 8, 12, 4), none, None, none, None,
                                   None) != 0
    assert b"vad_mlp_tail_backward: unsupported shape" in L.vad_last_error()
    assert L.vad_dense_forward_ex(None, 4, 8, None, None, 4, None, 1, 1.0, 0, 0, 0, 0, 0, None, 0, None) != 0
    assert b"vad_dense_forward_ex: unsupported shape" in L.vad_last_error()


def test_head_entry_points_refuse_before_any_launch():
    """vad_head_forward / vad_head_backward check shape, pointers, scratch size and alignment on the host, before
    anything is queued: a refused call returns non-zero with a text and needs no device."""
    from vad_amd import _native
    L = _native.lib()
    need = L.vad_head_scratch_floats(2, 3)
    names = [L.vad_cad_slot_name(i).decode() for i in range(L.vad_cad_num_slots())]
    slab = (L.vad_cad_slot_offset(names.index("direct_classifier.0.weight"))  # the first slot after the head
            - L.vad_cad_slot_offset(names.index("tracker.reid_net.0.weight")))
    assert need >= 2 * slab + 2 * 3 * 5 * (192 * 3 + 68) and L.vad_head_scratch_floats(3, 3) > need
    for B, T in [(0, 3), (2, 0), (2, 4097)]:
        assert L.vad_head_scratch_floats(B, T) < 0
        assert b"vad_head_scratch_floats: unsupported shape" in L.vad_last_error()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    a += -a % 16
    outs = [a] * 8
    fwd = lambda B, T, training, lg, par, scr, n: L.vad_head_forward(lg, B, T, par, training, 0, 0, 0, *outs, scr, n, None)
    bwd = lambda B, T, training, lg, par, scr, n, o=outs, g=a: L.vad_head_backward(
        lg, B, T, par, training, 0, 0, 0, *o, a, a, None, None, None, g, a, scr, n, None)
    for who, f in ((b"vad_head_forward", fwd), (b"vad_head_backward", bwd)):
        for args, text in [((0, 3, 1, a, a, a, need), b": unsupported shape"),
                           ((2, 4097, 1, a, a, a, need), b": unsupported shape"),
                           ((2, 3, 2, a, a, a, need), b": unsupported shape"),
                           ((2, 3, 1, None, a, a, need), b": null argument"),
                           ((2, 3, 1, a, None, a, need), b": null argument"),
                           ((2, 3, 1, a, a, None, need), b": scratch too small"),
                           ((2, 3, 1, a, a, a, need - 1), b": scratch too small"),
                           ((2, 3, 1, a, a, a + 4, need), b": params and scratch must be 16-byte aligned")]:
            assert f(*args) != 0
            assert who + text in L.vad_last_error(), (args, L.vad_last_error())
    assert L.vad_head_forward(a, 2, 3, a, 1, 0, 0, 0, *([a] * 7 + [None]), a, need, None) != 0
    assert b"vad_head_forward: null argument" in L.vad_last_error()
    assert bwd(2, 3, 1, a, a, a, need, g=None) != 0
    assert b"vad_head_backward: null argument" in L.vad_last_error()


def test_a2_head_entry_points_refuse_before_any_launch():
    """vad_a2_head_forward / vad_a2_head_backward check the plan and the flags on the host, before anything is queued:
    a refused call returns non-zero with a text and needs no device (creating a plan touches none)."""
    from vad_amd import _native
    L = _native.lib()
    h = ctypes.c_void_p()
    _native.check(L.vad_a2_create(2, 1, 4, 4, ctypes.byref(h)))  # the smallest clip: what the head tests run on
    try:
        fwd = lambda p: L.vad_a2_head_forward(p, None, 1, 0, 0, 0, 1, None, None, None, None, None, None)
        bwd = lambda p: L.vad_a2_head_backward(p, None, None, None, None, None, None)
        for who, call in ((b"vad_a2_head_forward", fwd), (b"vad_a2_head_backward", bwd)):
            assert call(None) != 0
            assert who + b": null plan" in L.vad_last_error()
            assert call(h) != 0
            assert who + b": plan not bound" in L.vad_last_error()
    finally:
        L.vad_a2_destroy(h)
    assert L.vad_a2_create(1, 1, 4, 4, ctypes.byref(h)) != 0 and L.vad_a2_create(257, 1, 4, 4, ctypes.byref(h)) != 0
    assert b"unsupported shape" in L.vad_last_error()


def test_mc_head_entry_points_refuse_before_any_launch():
    """vad_mc_head_forward / vad_mc_head_backward check the plan, the binding and the flags on the host, before
    anything is queued: a refused call returns non-zero with a text and needs no device (creating a plan touches
    none; the fake binding below is never dereferenced, because every call made on it is refused)."""
    from vad_amd import _native
    L = _native.lib()
    h = ctypes.c_void_p()
    _native.check(L.vad_mc_create(2, 1, 4, 8, 8, ctypes.byref(h)))  # the smallest clip: what the head tests run on
    try:
        fwd = lambda p, training=1, scores=None: L.vad_mc_head_forward(p, None, training, 0, 0, 0, None, scores,
                                                                        None, None, None, None)
        bwd = lambda p: L.vad_mc_head_backward(p, None, None, None, None)
        for who, call in ((b"vad_mc_head_forward", fwd), (b"vad_mc_head_backward", bwd)):
            assert call(None) != 0
            assert who + b": null plan" in L.vad_last_error()
            assert call(h) != 0
            assert who + b": plan not bound" in L.vad_last_error()
        fake = ctypes.c_void_p(256)
        _native.check(L.vad_mc_bind(h, fake, fake, fake, fake, None, fake, fake, fake))  # stores pointers only
        assert fwd(h, training=2, scores=fake) != 0
        assert b"vad_mc_head_forward: training is 0 or 1" in L.vad_last_error()
        assert fwd(h) != 0
        assert b"vad_mc_head_forward: null scores" in L.vad_last_error()
        assert bwd(h) != 0  # no head forward with labels on this plan, and no d_scores
        assert b"vad_mc_head_backward: no labels in the last head forward and no d_scores" in L.vad_last_error()
    finally:
        L.vad_mc_destroy(h)
    assert L.vad_mc_create(0, 1, 4, 8, 8, ctypes.byref(h)) != 0 and L.vad_mc_create(1025, 1, 4, 8, 8, ctypes.byref(h)) != 0
    assert b"unsupported shape" in L.vad_last_error()


def test_bbox_seam_entry_points_refuse_before_any_launch():
    """vad_bbox_head_forward / vad_bbox_debug_buffer check their arguments, the binding and the buffer name on the
    host, before anything is queued: a refused call returns non-zero with a text and needs no device (creating a plan
    touches none; the fake binding below is never dereferenced, because every call made on it is refused or only
    computes an address)."""
    from vad_amd import _native
    L = _native.lib()
    h = ctypes.c_void_p()
    _native.check(L.vad_bbox_create(2, 2, 2, 2, ctypes.byref(h)))  # the smallest clip: what the seam tests run on
    fake = ctypes.c_void_p(256)
    p, n = ctypes.c_void_p(), ctypes.c_int64()
    try:
        head = lambda plan, f=fake, s=fake, a=fake: L.vad_bbox_head_forward(plan, f, s, a, None)
        dbg = lambda plan, name=b"hc", pp=ctypes.byref(p), nn=ctypes.byref(n): L.vad_bbox_debug_buffer(plan, name, pp, nn)
        for who, call in ((b"vad_bbox_head_forward", head), (b"vad_bbox_debug_buffer", dbg)):
            assert call(None) != 0
            assert who + b": null argument" in L.vad_last_error()
            assert call(h) != 0
            assert who + b": plan not bound" in L.vad_last_error()
        _native.check(L.vad_bbox_bind(h, fake, fake))  # stores pointers only
        for kw in (dict(f=None), dict(s=None), dict(a=None)):
            assert head(h, **kw) != 0
            assert b"vad_bbox_head_forward: null argument" in L.vad_last_error()
        for kw in (dict(name=None), dict(pp=None), dict(nn=None)):
            assert dbg(h, **kw) != 0
            assert b"vad_bbox_debug_buffer: null argument" in L.vad_last_error()
        assert dbg(h, name=b"y3") != 0
        assert b"vad_bbox_debug_buffer: unknown buffer y3" in L.vad_last_error()
        sizes = dict(pooled=2 * 32, y2=2 * 64, hc=2 * 256, logits=2 * 256, hcl=2 * 128)
        for name, k in sizes.items():
            _native.check(dbg(h, name=name.encode()))
            assert n.value == k and p.value is not None and p.value >= 256, name
    finally:
        L.vad_bbox_destroy(h)
