"""The ctypes signatures of the kernel entry points are parsed from their C declarations (ops/_lib.py
parse_signatures).  A wrong one corrupts arguments silently on the GPU, so the parser is pinned from outside:
against a plain regex over the same files, against signatures written out by hand, and on synthetic input."""
import ctypes
import glob
import os
import re

import pytest

from pytorch_distributedtraining_amd.ops._lib import parse_signatures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, L, F, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_uint


def _sources():
    kernels = os.path.join(ROOT, "csrc", "kernels")
    files = glob.glob(os.path.join(kernels, "*.hip")) + glob.glob(os.path.join(kernels, "*.h"))
    return "".join(open(f).read() for f in sorted(files))


def _same(sig, restype, argtypes):
    """ctypes type identity, argument by argument."""
    return sig[0] is restype and len(sig[1]) == len(argtypes) and all(a is b for a, b in zip(sig[1], argtypes))


def test_whole_tree_parses_to_the_declared_names():
    sigs = parse_signatures()          # raises on an unmapped type or on disagreeing redeclarations
    names = re.findall(r"PDT_API (?:int|int64_t|long long) (pdt_\w+)\(", _sources())
    assert len(names) > 100
    assert set(sigs) == set(names), set(sigs) ^ set(names)
    assert len(sigs) == len(set(names))
    # redeclared names exist (prototype + definition), so agreement between declarations is exercised
    assert "pdt_gemm_stamps_epi_bf16" in {n for n in names if names.count(n) > 1}
    # the old argument-count check, by a plain split of the plain regex's argument list
    for m in re.finditer(r"PDT_API (?:int|int64_t|long long) (pdt_\w+)\(([^)]*)\)", _sources(), re.S):
        assert len(sigs[m.group(1)][1]) == len([a for a in m.group(2).split(",") if a.strip()]), m.group(1)


PINNED = {
    "pdt_adamw_mt": (I, [P, P, I, I, I, F, F, F, F, F, F, F, I, P, P, P, P]),
    "pdt_xgmi_collective": (I, [I, P, P, L, L, I, F, P, I, I, U, L, U, P, P]),
    "pdt_flash_attn_bwd": (I, [P, P, P, P, P, P, P, P, P, P, P, I, I, I, I, I, I, F, I, P, P, I, P, P]),
    "pdt_xgmi_ipc_handle_bytes": (I, []),
    "pdt_swin_mlp_ws_floats": (L, [I]),
    "pdt_fp8_gelu_bwd_ws_floats": (L, [I, I]),
    "pdt_win_attn_mfma_fwd": (I, [P, P, P, P, I, P, P, I, I, I, I, F, P, I, I, I, P]),
    "pdt_win_attn_mfma_bwd": (I, [P, P, P, P, I, P, P, P, P, P, I, I, I, I, F, I, P, I, P]),
    "pdt_win_attn_mfma_ok": (I, [I, I, I, I]),
    "pdt_window_perm": (I, [P, P, P, L, I, I, I, I, I, I, I, P]),
    "pdt_xgmi_alloc": (I, [L, I, P]),
    "pdt_gemm_stamps_epi_bf16": (I, [I, I, P, P, P, L, L, L, L, L, P, P, P, P]),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_signature(name):
    sig = parse_signatures()[name]
    assert _same(sig, *PINNED[name]), (name, sig)


def test_pins_cover_the_type_map():
    used = {t for _, args in PINNED.values() for t in args}
    assert used == {P, I, L, F, U}
    assert {r for r, _ in PINNED.values()} == {I, L}
    assert len(PINNED["pdt_flash_attn_bwd"][1]) == 24


def _one(decl):
    sigs = parse_signatures([decl])
    assert list(sigs) == ["pdt_f"], sigs
    return sigs["pdt_f"]


def test_synthetic_declarations():
    assert _same(_one("PDT_API int pdt_f(const float* const p);"), I, [P])
    assert _same(_one("PDT_API int pdt_f(const void* const* bufs, unsigned* e, void** out, hipStream_t st) { return 0; }"),
                 I, [P, P, P, P])
    assert _same(_one("PDT_API\nlong long\npdt_f(int64_t a,\n    const float b,\n  unsigned int c, uint32_t d,\n"
                      " unsigned e, long long g\n)\n{"), L, [L, F, U, U, U, L])
    assert _same(_one("PDT_API int pdt_f(int a,  // the first, with (parens) and a , comma\n"
                      "  /* a, b) */ float b /* int c, */) {"), I, [I, F])
    assert _same(_one("PDT_API int64_t pdt_f(void);"), L, [])
    assert _same(_one("PDT_API int pdt_f() { return 3; }"), I, [])
    # a commented-out declaration does not exist
    assert parse_signatures(["// PDT_API int pdt_g(int a);\n/* PDT_API int pdt_h(int a); */"]) == {}
    # the macro's own definition is not a declaration
    assert parse_signatures(['#define PDT_API extern "C" __attribute__((visibility("default")))\n']) == {}


def test_redeclarations():
    proto, defn = "PDT_API int pdt_f(const void* A, int64_t M, hipStream_t s);", \
                  "PDT_API int pdt_f(const void* a_ptr,\n int64_t rows, hipStream_t st) { return 0; }"
    assert _same(parse_signatures([proto + "\n" + defn])["pdt_f"], I, [P, L, P])
    assert _same(parse_signatures([proto, defn])["pdt_f"], I, [P, L, P])          # across files too
    for other in ("PDT_API int pdt_f(const void* A, int M, hipStream_t s);",      # an argument's type
                  "PDT_API int pdt_f(const void* A, int64_t M);",                 # the argument count
                  "PDT_API int64_t pdt_f(const void* A, int64_t M, hipStream_t s);"):   # the return width
        with pytest.raises(TypeError, match="pdt_f"):
            parse_signatures([proto, other])


@pytest.mark.parametrize("arg", ["double x", "size_t n", "bool b", "short h", "char c", "int64_t", "Foo f"])
def test_unmapped_argument_type_raises_and_names_it(arg):
    with pytest.raises(TypeError) as e:
        parse_signatures([f"PDT_API int pdt_f(int a, {arg}, float z);"])
    assert "pdt_f" in str(e.value) and f"'{arg}'" in str(e.value)


@pytest.mark.parametrize("ret", ["void", "float", "void*", "unsigned", "hipError_t"])
def test_unmapped_return_type_raises(ret):
    with pytest.raises(TypeError, match="pdt_f"):
        parse_signatures([f"PDT_API {ret} pdt_f(int a);"])


def test_64_bit_returns():
    wide = set(re.findall(r"PDT_API (?:int64_t|long long) (pdt_\w+)\(", _sources()))
    assert len(wide) >= 4
    sigs = parse_signatures()
    assert wide == {n for n, (ret, _) in sigs.items() if ret is ctypes.c_int64}      # 64-bit returns need c_int64
    assert all(ret is ctypes.c_int for n, (ret, _) in sigs.items() if n not in wide)
