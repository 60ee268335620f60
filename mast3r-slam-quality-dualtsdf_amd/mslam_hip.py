"""ctypes binding of libmslam_hip.so (C ABI declared in include/mslam_hip.h).

This is the only place that touches the shared library.  There is deliberately NO fallback: if the
library is missing, or a tensor is not resident on a HIP device, the call raises.
"""
import ctypes
import functools
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MSLAM_LIB", os.path.join(_HERE, "libmslam_hip.so"))   # MSLAM_LIB: measurement builds (tools/probes)

_HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "mslam_hip.h"))

# by-value parameter types the header may use; any parameter with a `*` is passed as an address
_SCALARS = {
    "int": ctypes.c_int,
    "float": ctypes.c_float,
    "double": ctypes.c_double,
    "size_t": ctypes.c_size_t,
    "long long": ctypes.c_longlong,
    "int64_t": ctypes.c_int64,
    "uint64_t": ctypes.c_uint64,
    "uint32_t": ctypes.c_uint32,
}
_RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p}


def _argtype(fn: str, param: str):
    if "*" in param and "(" not in param:   # any data pointer; a function pointer falls through and is refused
        return ctypes.c_void_p
    words = [w for w in param.split() if w != "const"]
    ctype = _SCALARS.get(" ".join(words[:-1]))   # the last word is the parameter's name
    if ctype is None or not re.fullmatch(r"\w+", words[-1]):   # `float v[3]` is a pointer in C: write it as one
        raise ValueError(f"{fn}: unsupported parameter '{param}'")
    return ctype


def parse_header(text: str) -> dict:
    """{name: (restype, [argtypes])} of every `<ret> mslam_<name>(<params>);` in the header text.

    Anything outside the closed type maps above raises ValueError: a default would load, run and hand
    the callee garbage."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', ";", text).replace("}", ";")   # the header's only braces are the C++ guard's
    out = {}
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split())
        if not stmt:
            continue
        m = re.fullmatch(r"([\w *]+?) ?\b(mslam_\w+) ?\((.*)\)", stmt)
        if m is None:
            raise ValueError(f"not a plain declaration of an mslam_ function: '{stmt}'")
        ret, fn, params = m.group(1).replace(" *", "*"), m.group(2), m.group(3).strip()
        restype = _RETURNS.get(ret)
        if restype is None:
            raise ValueError(f"{fn}: unsupported return type '{ret}'")
        plist = [] if params in ("", "void") else [q.strip() for q in params.split(",")]
        out[fn] = (restype, [_argtype(fn, q) for q in plist])
    return out


@functools.lru_cache(maxsize=None)
def _header_text() -> str:
    """include/mslam_hip.h, read once."""
    if not os.path.exists(_HEADER_PATH):
        raise RuntimeError(
            f"{_HEADER_PATH} not found: the binding reads every signature from the header that "
            "libmslam_hip.so is built against. There is no hand-written copy to fall back to."
        )
    with open(_HEADER_PATH) as f:
        return f.read()


def header_constants(text: str = None) -> dict:
    """{name: int} of every `#define MSLAM_<NAME> <integer or (negative integer)>` of include/mslam_hip.h (or `text`),
    so that no Python module keeps a copy; a define of anything else (a float, an expression, a macro) is left out."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", _header_text() if text is None else text, flags=re.S)
    value = r"(\d+|\([ \t]*-[ \t]*\d+[ \t]*\))"
    found = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(MSLAM_\w+)[ \t]+" + value + r"[ \t]*$", text, flags=re.M)
    return {name: int(re.sub(r"[() \t]", "", v)) for name, v in found}


def exported_symbols():
    """Every symbol include/mslam_hip.h declares (used by the CPU-side ABI test)."""
    return sorted(parse_header(_header_text()))


_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback for this path."
            )
        handle = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in parse_header(_header_text()).items():
            fn = getattr(handle, name)
            fn.argtypes = argtypes
            fn.restype = restype
        _lib = handle
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().mslam_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")


def stream_ptr() -> int:
    """hipStream_t of torch's current stream on the current device."""
    return torch.cuda.current_stream().cuda_stream


def ptr(t) -> int:
    """Device pointer of a tensor (None -> NULL).  Raises for host tensors: no CPU path exists."""
    if t is None:
        return 0
    if not t.is_cuda:
        raise RuntimeError(
            "libmslam_hip.so operates on HIP device tensors only; got a tensor on "
            f"{t.device}. There is no CPU fallback."
        )
    return t.data_ptr()


def require_contiguous(**tensors) -> None:
    """Mirror of CHECK_CONTIGUOUS (mast3r_slam/backend/include/gn.h:5): RuntimeError by name."""
    for name, t in tensors.items():
        if not t.is_contiguous():
            raise RuntimeError(f"{name} must be contiguous")


def require_dtype(t, dtype, name: str) -> None:
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must have dtype {dtype}, got {t.dtype}")
