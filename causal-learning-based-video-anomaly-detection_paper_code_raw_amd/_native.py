"""ctypes binding of libvadhip.so (the C ABI in include/vad.h).

The signatures are read from the header at import (_parse_header), so a new entry point is declared in vad.h and
nowhere else; the .hip files include the same header, which ties the definitions to it.

There is no fallback: if the library is missing or no HIP device is present, every entry point raises.
"""
from __future__ import annotations

import ctypes
import os
import re

_LIB = None
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libvadhip.so")
HEADER_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "vad.h")

# int (*vad_bn_sync_fn)(void* user, int bn_layer, int phase, int64_t n, void* stream)
BN_SYNC_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                              ctypes.c_void_p)

# header type -> ctypes class.  Every pointer not listed here is a c_void_p, out-parameters included: a c_void_p takes
# an address, None, ctypes.byref(...) and ctypes arrays alike.
_CTYPES = {
    "int": ctypes.c_int,
    "int64_t": ctypes.c_int64,
    "uint64_t": ctypes.c_uint64,
    "uint32_t": ctypes.c_uint32,
    "float": ctypes.c_float,
    "double": ctypes.c_double,
    "const char*": ctypes.c_char_p,
    "vad_bn_sync_fn": BN_SYNC_FN,
}


def _ctype(fn: str, ctype: str):
    t = re.sub(r"\s*\*\s*", "*", " ".join(ctype.split()))
    if t in _CTYPES:
        return _CTYPES[t]
    if re.fullmatch(r"\w[\w *]*\*", t):
        return ctypes.c_void_p
    raise ValueError(f"vad.h: {fn}: unknown type {t!r}")


def _parse_header(text: str) -> dict:
    """{name: (restype, [argtypes])} of every `ret vad_name(params);` declaration of a vad.h text.  It knows what vad.h
    holds and nothing more; a declaration or a type outside that raises."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    lines = [ln for ln in text.splitlines() if not re.match(r'\s*(#|typedef\b|extern "C"|}\s*$)', ln)]
    sigs = {}
    for decl in " ".join(lines).split(";"):
        if not decl.strip():
            continue
        m = re.fullmatch(r"\s*(.+?)\b(vad_\w+)\s*\((.*)\)\s*", decl)
        if not m or m.group(2) in sigs:
            raise ValueError(f"vad.h: cannot parse {decl.strip()!r}")
        ret, name, params = m.groups()
        args = []
        for p in params.split(",") if params.strip() != "void" else []:
            pm = re.fullmatch(r"\s*(.*[\s*])\w+\s*", p)  # the type, then the parameter's name
            if not pm:
                raise ValueError(f"vad.h: {name}: cannot parse parameter {p.strip()!r}")
            args.append(_ctype(name, pm.group(1)))
        sigs[name] = (None if ret.strip() == "void" else _ctype(name, ret), args)
    return sigs


with open(HEADER_PATH) as _f:
    _SIGS = _parse_header(_f.read())


def lib():
    """Load libvadhip.so (after torch, so both share one HIP runtime)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    import torch  # noqa: F401  (loads torch's libamdhip64.so.7 first)
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"libvadhip.so is not built ({LIB_PATH}); run __graft_entry__.build()")
    L = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        try:
            fn = getattr(L, name)
        except AttributeError:  # (an older build, e.g. an A/B baseline: calling the entry point raises then)
            continue
        fn.restype = res
        fn.argtypes = args
    if L.vad_abi_version() != 1:
        raise RuntimeError("libvadhip ABI mismatch")
    _LIB = L
    return L


def check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError("libvadhip: " + lib().vad_last_error().decode())


def ptr(t) -> int | None:
    return None if t is None else t.data_ptr()


def stream_of(device) -> int:
    import torch
    return torch.cuda.current_stream(device).cuda_stream


def require_hip(t) -> None:
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError("this build runs on MI355X (HIP) devices only; got a tensor on "
                           f"{getattr(t, 'device', type(t))}")


def host_device_ptr(t) -> int:
    """Device address of a pinned host tensor (kernels write it over PCIe; vad_host_device_ptr)."""
    if not t.is_pinned():
        raise ValueError("host_device_ptr: the tensor must be pinned")
    out = ctypes.c_void_p()
    check(lib().vad_host_device_ptr(t.data_ptr(), ctypes.addressof(out)))
    return out.value
