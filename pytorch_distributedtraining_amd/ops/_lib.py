"""ctypes binding of ``lib/libpdt_kernels.so`` (the gfx950 HIP kernels).

The library is loaded lazily, after ``import torch``, so its ``libamdhip64.so.7`` dependency resolves
to the HIP runtime torch already mapped (one runtime, one set of streams).  Every entry point takes
raw device pointers plus the current HIP stream handle and returns a ``hipError_t``.

Policy: a GPU tensor ALWAYS goes through the HIP kernels -- if the library is missing on a GPU box
the op raises (no silent eager fallback).  CPU tensors use the PyTorch reference math; that path
exists for the CPU unit tests and the gloo multi-process tests.
"""
from __future__ import annotations

import ctypes
import glob
import os
import re
import threading

import torch

# PDT_KERNEL_LIB points at another build of the library (A/B of two kernel builds on one box)
_LIB_PATH = os.environ.get("PDT_KERNEL_LIB") or os.path.join(
    os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lib", "libpdt_kernels.so")
_lock = threading.Lock()
_lib = None
_load_error: Exception | None = None

c_void_p = ctypes.c_void_p
c_int = ctypes.c_int
c_int64 = ctypes.c_int64
c_float = ctypes.c_float

# The bindings are read off the C declarations themselves (csrc/kernels ships with the tree and the library is
# built from it), so a signature exists in one place only.  Strict on purpose: a C type that is not listed here
# raises instead of falling through to a default -- a wrong argtype does not fail, it corrupts the argument.
_KERNEL_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))),
                           "csrc", "kernels")
_ARG_TYPES = {"hipStream_t": c_void_p, "int": c_int, "int64_t": c_int64, "long long": c_int64, "float": c_float,
              "unsigned": ctypes.c_uint, "unsigned int": ctypes.c_uint, "uint32_t": ctypes.c_uint}
_RET_TYPES = {"int": c_int, "int64_t": c_int64, "long long": c_int64}
_DECL = re.compile(r"\bPDT_API\s+([^()]*?)\s*\b(pdt_\w+)\s*\(([^()]*)\)")


def parse_signatures(texts=None) -> dict:
    """``{name: (restype, [argtypes])}`` of every ``PDT_API <ret> pdt_<name>(<args>)`` -- prototype or definition --
    in ``texts`` (default: the ``*.hip`` and ``*.h`` kernel sources).  A name may be declared more than once only
    with one signature."""
    if texts is None:
        texts = []
        for ext in ("*.hip", "*.h"):
            for path in sorted(glob.glob(os.path.join(_KERNEL_SRC, ext))):
                with open(path) as f:
                    texts.append(f.read())
    sigs = {}
    for text in texts:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
        for ret, name, args in _DECL.findall(text):
            ret = " ".join(ret.split())
            if ret not in _RET_TYPES:
                raise TypeError(f"{name}: return type '{ret}' has no ctypes mapping")
            argtypes = []
            for arg in ([] if args.strip() in ("", "void") else args.split(",")):
                if "*" in arg:
                    argtypes.append(c_void_p)
                    continue
                ctype = " ".join([w for w in arg.split() if w != "const"][:-1])     # all but the argument's name
                if ctype not in _ARG_TYPES:
                    raise TypeError(f"{name}: argument '{' '.join(arg.split())}' has no ctypes mapping")
                argtypes.append(_ARG_TYPES[ctype])
            sig = (_RET_TYPES[ret], argtypes)
            if sigs.setdefault(name, sig) != sig:
                raise TypeError(f"{name}: declared twice with different signatures")
    return sigs


F32, BF16, F16, F64 = 0, 1, 2, 3


def dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float32:
        return F32
    if dt == torch.bfloat16:
        return BF16
    if dt == torch.float16:
        return F16
    if dt == torch.float64:
        return F64
    raise TypeError(f"unsupported dtype for HIP kernel: {dt}")


def lib_path() -> str:
    return _LIB_PATH


def load():
    """Return the loaded kernel library (raises if it cannot be loaded)."""
    global _lib, _load_error
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(_LIB_PATH):
            _load_error = FileNotFoundError(
                f"{_LIB_PATH} missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or python -m pytorch_distributedtraining_amd._build)")
            raise _load_error
        lib = ctypes.CDLL(_LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        for name, (restype, argtypes) in parse_signatures().items():
            fn = getattr(lib, name, None)
            if fn is None:
                continue
            fn.argtypes = argtypes
            fn.restype = restype
        _lib = lib
        return _lib


def available() -> bool:
    """True when a GPU is present and the HIP kernel library loads."""
    if not torch.cuda.is_available():
        return False
    try:
        load()
        return True
    except Exception:  # pragma: no cover - reported by require()
        return False


def require():
    """The kernel library, or a loud error (used by every GPU code path)."""
    try:
        return load()
    except Exception as e:  # pragma: no cover
        raise RuntimeError(f"pytorch_distributedtraining_amd HIP kernels unavailable: {e}") from e


def stream_handle(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def ptr(t) -> int:
    return 0 if t is None else t.data_ptr()


def check(err: int, name: str) -> None:
    if err != 0:
        raise RuntimeError(f"HIP kernel {name} failed with hipError_t={err}")


def call(name: str, *args) -> None:
    lib = require()
    check(getattr(lib, name)(*args), name)
