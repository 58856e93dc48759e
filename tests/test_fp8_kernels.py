"""The fp8 cast kernels (csrc/kernels/fp8.hip, the quant / dequant kernels of elementwise.hip) tested directly:
exact rounding over every bf16 bit pattern, the NaN / inf contract shared with the torch fallback of ops/fp8.py,
the fused bias-GELU casts against a float64 reference of their own operation, and the device scale update
against the CPU path.  The reference conversion (tests/fp8_ref.py) is built from the decode table alone."""
import types

import pytest
import torch

from fp8_ref import FMT_DTYPE, FMT_MAX, all_bf16_patterns, code_order, decode_table, ref_quant
from pytorch_distributedtraining_amd.ops import fp8 as F8

BF16, F32 = torch.bfloat16, torch.float32
SCALES = {"1": 1.0, "2^-7": 2.0 ** -7, "0.37": 0.37}
NFINITE = {0: 0x7E, 1: 0x7B}                      # largest magnitude code that is a finite value
# Observed on MI355X, identical for the 64-tile kernel, the 128-tile kernel and pdt_fp8_quant (vector body and
# scalar tail), bf16 and fp32 inputs:       e4m3fn          e5m2
#   NaN (either sign, quiet or signalling)   0xff            0xfe
#   +inf / -inf, and finite x whose          0x7f / 0xff     0x7c / 0xfc
#     x * scale overflows fp32               (NaN codes)     (inf codes)
# The GPU tests below take their expected bytes from the torch fallback, which is built to match; only the CPU
# test of that fallback names the NaN code.
NAN_CODE = {0: 0xFF, 1: 0xFE}


def u8(t):
    return t.view(torch.uint8)


def _meta(dev, scale, slot=0):
    m = F8.Fp8Meta(dev)
    m.scale[slot] = scale
    return m


def _amax_no_nan(x):
    xf = x.float().abs()
    return torch.where(torch.isnan(xf), torch.zeros_like(xf), xf).max()


# ---------------------------------------------------------------------------------------------------------------
# 1. the reference itself (CPU)
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("scale", [1.0, 0.37, 2.0 ** -7, 2.0 ** 9, 3.0])
def test_ref_quant_matches_torch_cpu(fmt, scale):
    """All 65536 bf16 bit patterns: wherever the scaled fp32 value is finite, ref_quant equals torch's CPU
    conversion byte for byte (two independent constructions of round-to-nearest-even with saturation)."""
    x = all_bf16_patterns()
    p = x.float() * torch.tensor(scale, dtype=F32)
    fin = torch.isfinite(p)
    want = u8(p.clamp(-FMT_MAX[fmt], FMT_MAX[fmt]).to(FMT_DTYPE[fmt]))
    got = ref_quant(p.double(), fmt)
    assert 62000 < int(fin.sum()) <= 65536 - 256           # 2 x 128 NaN / inf patterns, plus overflow at 2^9
    assert torch.equal(got[fin], want[fin])
    # +-inf saturate
    assert ref_quant(torch.tensor([float("inf"), -float("inf")], dtype=torch.float64), fmt).tolist() == \
        [NFINITE[fmt], NFINITE[fmt] | 0x80]


@pytest.mark.parametrize("fmt", [0, 1])
def test_ref_quant_ties_and_code_order_cpu(fmt):
    tab = decode_table(fmt)
    n = NFINITE[fmt]
    codes = torch.arange(n + 1, dtype=torch.uint8)
    assert torch.equal(ref_quant(tab[: n + 1], fmt), codes)                   # representable values: themselves
    assert torch.equal(ref_quant(-tab[: n + 1], fmt), codes | 0x80)           # -0 keeps its sign
    mid = (tab[:n] + tab[1: n + 1]) / 2                                       # exact ties -> the even neighbour
    even = codes[:n] + (codes[:n] % 2)
    assert torch.equal(ref_quant(mid, fmt), even)
    eps = mid * 2.0 ** -40
    assert torch.equal(ref_quant(mid - eps, fmt), codes[:n]) and torch.equal(ref_quant(mid + eps, fmt), codes[:n] + 1)
    allc = torch.arange(256, dtype=torch.uint8)
    fin = torch.isfinite(tab)
    o = code_order(allc)[fin]
    srt = torch.argsort(tab[fin], stable=True)
    assert bool((o[srt][1:] >= o[srt][:-1]).all())                            # monotone in the decoded value
    assert int(code_order(torch.tensor([0x80], dtype=torch.uint8))) == 0


# ---------------------------------------------------------------------------------------------------------------
# 3 (CPU half). the torch fallback keeps the kernels' contract: finite scaled values saturate, NaN / +-inf scaled
# values are converted unclamped, amax ignores NaN
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("scale", [1.0, 0.37])
def test_fallback_contract_cpu(fmt, scale):
    x = all_bf16_patterns().view(256, 256)
    meta = _meta("cpu", scale)
    q, qt = F8.cast_transpose(x, meta, 0, fmt)
    p = x.float() * meta.scale[0]
    fin = torch.isfinite(p)
    inf, nan = torch.isinf(p), torch.isnan(p)
    assert torch.equal(u8(q)[fin], ref_quant(p.double(), fmt)[fin])
    assert torch.equal(u8(q)[inf], u8(p.to(FMT_DTYPE[fmt]))[inf])            # not clamped to +-fmax
    assert bool((u8(q)[nan] == NAN_CODE[fmt]).all()) and int(nan.sum()) >= 254
    assert bool(torch.isnan(decode_table(fmt)[NAN_CODE[fmt]]))
    assert torch.equal(u8(qt), u8(q).t())
    assert float(meta.cur[0]) == float("inf")                                # +-inf counts, NaN does not
    xn = x.clone()
    xn[torch.isinf(xn)] = 2.0
    meta = _meta("cpu", scale)
    F8.cast_transpose(xn, meta, 0, fmt, want_q=False, want_t=False)
    assert float(meta.cur[0]) == float(_amax_no_nan(xn)) == float(torch.finfo(BF16).max)
    if fmt == 0:
        amax = torch.zeros(1)
        qq = F8.quantize_fp8(xn.view(-1), meta.scale[0:1], amax)
        pn = xn.float().view(-1) * meta.scale[0]
        finn = torch.isfinite(pn)
        assert torch.equal(qq[finn], ref_quant(pn.double(), 0)[finn])
        assert torch.equal(qq[torch.isinf(pn)], u8(pn.to(FMT_DTYPE[0]))[torch.isinf(pn)])
        assert bool((qq[torch.isnan(pn)] == NAN_CODE[0]).all())
        assert float(amax) == float(torch.finfo(BF16).max)


# ---------------------------------------------------------------------------------------------------------------
# 2. exhaustive rounding of the plain cast kernels (GPU, exact)
# ---------------------------------------------------------------------------------------------------------------

def _patterns_2d(shape, dt, dev="cuda"):
    R, C = shape
    pat = all_bf16_patterns(dev)
    idx = torch.arange(R * C, device=dev) % 65536           # (192, 384): the 8192 padding elements repeat
    return pat[idx].view(R, C).to(dt).contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("scale", list(SCALES.values()), ids=list(SCALES))
@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", [(256, 256), (192, 384)], ids=["tile128", "tile64"])
def test_cast_transpose_all_bf16_patterns(shape, dt, fmt, scale):
    """Every bf16 value (as bf16, and widened to fp32) through both tile kernels.  Scale 1 keeps every tie, both
    saturation boundaries and +-0; 2^-7 pushes a large share into fp8 subnormals and to +-0; 0.37 is generic."""
    x = _patterns_2d(shape, dt)
    meta = _meta("cuda", scale)
    q, qt = F8.cast_transpose(x, meta, 0, fmt)
    p = x.float() * meta.scale[0]
    fin = torch.isfinite(p)
    ref = ref_quant(p.double(), fmt)
    assert torch.equal(u8(q)[fin], ref[fin])
    assert torch.equal(u8(qt), u8(q).t())
    assert float(meta.cur[0]) == float(_amax_no_nan(x)) == float("inf")


@pytest.mark.gpu
@pytest.mark.parametrize("scale", list(SCALES.values()), ids=list(SCALES))
@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "f32"])
def test_quantize_fp8_all_bf16_patterns(dt, scale):
    pat = all_bf16_patterns("cuda")
    tail = pat[torch.tensor([0x8000, 0x3F80, 0x43E0, 0xC3E8, 0x0001], device="cuda")]   # -0 1 448 -464 denormal
    x = torch.cat([pat, tail]).to(dt)                      # 65536 + 5: the last 5 go through the scalar tail loop
    sc = torch.tensor([scale], dtype=F32, device="cuda")
    amax = torch.zeros(1, device="cuda")
    q = F8.quantize_fp8(x, sc, amax)
    p = x.float() * sc
    fin = torch.isfinite(p)
    assert q.shape == x.shape and int(fin[-5:].sum()) == 5
    assert torch.equal(q[fin], ref_quant(p.double(), 0)[fin])
    assert float(amax) == float("inf")
    # the same without the +-inf inputs: a finite amax, NaN inputs ignored
    xf = torch.where(torch.isinf(x), torch.ones_like(x), x)
    amax.zero_()
    F8.quantize_fp8(xf, sc, amax)
    assert float(amax) == float(_amax_no_nan(xf)) == float(torch.finfo(BF16).max)


@pytest.mark.gpu
@pytest.mark.parametrize("si", [1.0, 0.5])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_dequantize_fp8_all_codes(dt, si):
    codes = (torch.arange(256 * 5 + 3, device="cuda") % 256).to(torch.uint8)
    y = F8.dequantize_fp8(codes, torch.tensor([si], dtype=F32, device="cuda"), dt)
    want = (decode_table(0, "cuda").float()[codes.long()] * torch.tensor(si, dtype=F32, device="cuda")).to(dt)
    nan = torch.isnan(want)
    assert y.dtype == dt and torch.equal(torch.isnan(y), nan)
    assert torch.equal(nan, (codes & 0x7F) == 0x7F)        # 0x7f and 0xff come back as NaN, nothing else does
    assert torch.equal(u8(y[~nan].contiguous()), u8(want[~nan].contiguous()))   # bit-exact, signed zeros included


# ---------------------------------------------------------------------------------------------------------------
# 3. non-finite contract: the three kernel families and the torch fallback produce the same bytes and amax
# ---------------------------------------------------------------------------------------------------------------

_SPECIAL_BITS = {                                   # fp32 bit patterns planted into an otherwise ordinary tensor
    "nan": [0x7FC00000, 0xFFC00000, 0x7F810000, 0xFFFF0000],     # +-quiet, signalling, all-ones payload (bf16-exact)
    "inf": [0x7F800000, 0xFF800000],
    "overflow": [0x7F000000, 0xFF000000, 0x7F7F0000, 0xFF7F0000],   # +-2^127, +-bf16 max: finite, x * 4 is not
}


def _special_input(kind, numel, dt):
    g = torch.Generator().manual_seed(99)
    x = (torch.randn(numel, generator=g) * 3).to(dt)
    bits = _SPECIAL_BITS[kind]
    pos = [0, 1, 7, 8, 63, 64, 65, 127, 128, numel // 2 + 3, numel - 129, numel - 65, numel - 9, numel - 2, numel - 1]
    xi = x.view(torch.int32 if dt == F32 else torch.int16)  # planted as bits: a value cast would canonicalise NaN
    for k, i in enumerate(pos):
        b = bits[k % len(bits)] if dt == F32 else bits[k % len(bits)] >> 16
        top = 1 << (32 if dt == F32 else 16)
        xi[i] = b - top if b >= top // 2 else b
    return x, torch.tensor(pos)


# Observed codes: the table next to NAN_CODE at the top of this file.
@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(_SPECIAL_BITS))
@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", [(256, 256), (192, 384)], ids=["tile128", "tile64"])
def test_nonfinite_cast_transpose_matches_fallback(shape, dt, fmt, kind):
    R, C = shape
    xc, pos = _special_input(kind, R * C, dt)
    xc = xc.view(R, C)
    scale = 4.0 if kind == "overflow" else 0.37
    mg, mc = _meta("cuda", scale), _meta("cpu", scale)
    q, qt = F8.cast_transpose(xc.cuda(), mg, 0, fmt)
    qc, qtc = F8.cast_transpose(xc, mc, 0, fmt)             # CPU tensor: the torch fallback
    got = u8(q).cpu()
    print(kind, shape, dt, fmt, "codes at the planted positions:", [hex(v) for v in got.view(-1)[pos].tolist()],
          "amax", float(mg.cur[0]))
    assert not torch.isfinite(xc.float() * mc.scale[0]).view(-1)[pos].any()
    assert torch.equal(got, u8(qc))
    assert torch.equal(u8(qt).cpu(), u8(qtc))
    assert torch.equal(mg.cur.cpu(), mc.cur)
    assert float(mc.cur[0]) == float(_amax_no_nan(xc))
    # amax-only form
    mg.cur.zero_()
    F8.cast_transpose(xc.cuda(), mg, 0, fmt, want_q=False, want_t=False)
    assert torch.equal(mg.cur.cpu(), mc.cur)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(_SPECIAL_BITS))
@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "f32"])
def test_nonfinite_quantize_matches_fallback(dt, kind):
    xc, pos = _special_input(kind, 4096 + 5, dt)            # the last two planted values are in the scalar tail
    scale = 4.0 if kind == "overflow" else 0.37
    sg, ag = torch.tensor([scale], device="cuda"), torch.zeros(1, device="cuda")
    sc, ac = torch.tensor([scale]), torch.zeros(1)
    q = F8.quantize_fp8(xc.cuda(), sg, ag)
    qc = F8.quantize_fp8(xc, sc, ac)
    print(kind, dt, "codes at the planted positions:", [hex(v) for v in q.cpu()[pos].tolist()], "amax", float(ag))
    assert torch.equal(q.cpu(), qc)
    assert torch.equal(ag.cpu(), ac) and float(ac) == float(_amax_no_nan(xc))
    # the tile kernels give the same bytes for the same values (64 x 64 of them)
    m = _meta("cuda", scale)
    q2, _ = F8.cast_transpose(xc[-4096:].view(64, 64).cuda(), m, 0, 0)
    assert torch.equal(u8(q2).view(-1), q[-4096:])


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("family", ["tile128", "tile64", "quant"])
def test_amax_survives_signalling_nan(family, dt):
    """The tensor's maximum sits right before a signalling NaN in the same lane's run of elements.  A bare
    v_max3_f32 returns a quiet NaN for a signalling operand and the next max drops it with the running amax: the
    128-tile kernel and pdt_fp8_quant used to report 1.0 here instead of 1000."""
    shape = {"tile128": (256, 256), "tile64": (192, 384), "quant": (4096 + 5,)}[family]
    x = torch.ones(shape, dtype=dt)
    flat = x.view(-1)
    xi = flat.view(torch.int32 if dt == F32 else torch.int16)
    for i in (2, 1000, flat.numel() // 2 + 4):             # even: the value and its NaN share one max3
        flat[i] = 1000.0
        xi[i + 1] = 0x7F810000 if dt == F32 else 0x7F81
    if family == "quant":
        amax = torch.zeros(1, device="cuda")
        F8.quantize_fp8(x.cuda(), torch.ones(1, device="cuda"), amax)
        assert float(amax) == 1000.0
    else:
        for wq in (True, False):
            meta = _meta("cuda", 1.0)
            F8.cast_transpose(x.cuda(), meta, 0, 0, want_q=wq, want_t=wq)
            assert float(meta.cur[0]) == 1000.0


# ---------------------------------------------------------------------------------------------------------------
# 4. fused bias-GELU casts against a float64 reference of the same operation
# ---------------------------------------------------------------------------------------------------------------
#
# shape -> the path it reaches (tile kernel picked by divisibility; the grid is capped at 2048 blocks)
GELU_SHAPES = [
    (192, 320),      # 64-tile kernel, one tile per block
    (128, 192),      # R a multiple of 128 but C not: still the 64-tile kernel
    (256, 384),      # 128-tile kernel
    (4160, 2112),    # 65 x 33 = 2145 tiles of 64 > 2048: some blocks do two tiles (prefetch, LDS reuse)
    (8320, 4224),    # 2145 tiles of 128: the same for the 128-tile kernel
]
MARGIN = 8.0         # allowance over the measured fp32-formula error for the kernels' __expf / rcp intrinsics
DIST1_CAP = 1e-3     # share of elements one code away from the float64 reference (a condition, not a measurement)
# Measured on MI355X (max code distance / share at distance 1; no element was ever further than 1):
#   shape        fwd e4m3      fwd e5m2   bwd e5m2      bwd e4m3
#   192x320      0 / 0         0 / 0      0 / 0         0 / 0
#   128x192      0 / 0         -          0 / 0         -
#   256x384      1 / 7.1e-5    0 / 0      1 / 2.0e-5    1 / 1.0e-5
#   4160x2112    0 / 0         -          1 / 6.8e-7    -
#   8320x4224    0 / 0         -          1 / 5.1e-7    -
# (the kernels' sigmoid form evaluated in plain fp32 on the CPU gives 0 forward and 1e-7 .. 2e-6 backward).
# Formula error of a plain fp32 torch evaluation against float64, max over the five shapes (computed again for
# the actual inputs in gelu_case): amax forward 4.9e-8, amax backward 4.4e-7, column sums 2.7e-7.  The kernels'
# own amax error was 0 forward (at the maximum gelu(u) = u to fp32 precision) and <= 6.8e-8 backward.


@pytest.fixture(scope="module", params=GELU_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def gelu_case(request):
    """Inputs, the float64 references of both fused operations, and the error of a plain fp32 torch evaluation of
    the same formulas against them (the yardstick for the amax / dbias tolerances).  Built once per shape."""
    R, C = request.param
    g = torch.Generator(device="cuda").manual_seed(R * 10007 + C)
    a = (torch.randn(R, C, device="cuda", generator=g) * 2).bfloat16()
    bias = (torch.randn(C, device="cuda", generator=g) * 0.5).bfloat16()
    dh = torch.randn(R, C, device="cuda", generator=g).bfloat16()
    u = a.double() + bias.double()
    vf = F8._gelu_tanh(u)
    vb = dh.double() * F8._gelu_tanh_grad(u)
    u32 = a.float() + bias.float()
    ef = (F8._gelu_tanh(u32).double() - vf).abs()
    eb = (dh.float() * F8._gelu_tanh_grad(u32)).double().sub_(vb).abs_()
    del u, u32
    c = types.SimpleNamespace(R=R, C=C, a=a, bias=bias, dh=dh, vf=vf, vb=vb)
    c.amax_f, c.amax_b = float(vf.abs().max()), float(vb.abs().max())
    # |max|v32| - max|v64|| <= max|v32 - v64|: the sup-norm formula error, relative to amax, bounds the amax error
    c.e_amax_f, c.e_amax_b = float(ef.max()) / c.amax_f, float(eb.max()) / c.amax_b
    c.db_ref, c.db_S = vb.sum(0), vb.abs().sum(0)
    # |sum_i v32_ij - sum_i v64_ij| <= sum_i |v32_ij - v64_ij| =: e_j * S_j: the formula error of a column sum
    c.e_col = float((eb.sum(0) / c.db_S).max())
    print(f"gelu_case {R}x{C}: fp32 formula error  amax fwd {c.e_amax_f:.3e}  amax bwd {c.e_amax_b:.3e}  "
          f"column sums {c.e_col:.3e}")
    return c


def _check_codes(name, q, ref, fmt):
    """Every code finite, at most one representable step from the float64 reference, and only a small share there."""
    qb = u8(q)
    assert int((qb & 0x7F).max()) <= NFINITE[fmt], f"{name}: NaN / inf code in the output"
    d = (code_order(qb) - code_order(ref)).abs()
    dmax, share = int(d.max()), float((d == 1).double().mean())
    print(f"{name}: max code distance {dmax}, share at distance 1 {share:.3e}")
    # measured shares: the table at DIST1_CAP (worst 7.1e-5)
    assert dmax <= 1, f"{name}: {int((d > 1).sum())} elements more than one code from the reference (max {dmax})"
    assert share <= DIST1_CAP, f"{name}: share at distance 1 {share:.3e}"


def _gelu_fwd(case, fmt):
    fmax = FMT_MAX[fmt]
    out = {}
    for wq, wt in [(True, True), (True, False), (False, True), (False, False)]:
        meta = _meta("cuda", fmax / case.amax_f)
        q, qt = F8.bias_gelu_cast_transpose(case.a, case.bias, meta, 0, fmt, want_q=wq, want_t=wt)
        assert (q is not None) == wq and (qt is not None) == wt
        out[wq, wt] = (q, qt, float(meta.cur[0]), meta.scale[0].double())
    q, qt, cur, sc = out[True, True]
    assert q.shape == (case.R, case.C) and qt.shape == (case.C, case.R) and q.dtype == FMT_DTYPE[fmt]
    assert torch.equal(u8(qt), u8(q).t())
    assert torch.equal(u8(out[True, False][0]), u8(q))
    assert torch.equal(u8(out[False, True][1]), u8(qt))
    _check_codes(f"gelu fwd {case.R}x{case.C} fmt{fmt}", q, ref_quant(case.vf * sc, fmt), fmt)
    # amax of the GELU output: measured fp32 formula error (e_amax_f, ~5e-8 at these shapes) times MARGIN
    tol = MARGIN * case.e_amax_f
    print(f"gelu fwd {case.R}x{case.C}: amax rel err {abs(cur - case.amax_f) / case.amax_f:.3e} (tol {tol:.3e})")
    assert abs(cur - case.amax_f) <= tol * case.amax_f
    assert all(o[2] == cur for o in out.values())           # q-only, qt-only and amax-only leave the same amax


def _gelu_bwd(case, fmt):
    fmax = FMT_MAX[fmt]
    out = {}
    for wq, wt, wdb in [(True, True, True), (True, True, False), (True, False, True), (False, True, True),
                        (False, False, True), (False, False, False)]:
        meta = _meta("cuda", fmax / case.amax_b)
        q, qt, db = F8.bias_gelu_bwd_cast_transpose(case.dh, case.a, case.bias, meta, 0, fmt, want_q=wq, want_t=wt,
                                                    want_db=wdb)
        assert (q is not None) == wq and (qt is not None) == wt and (db is not None) == wdb
        out[wq, wt, wdb] = (q, qt, db, float(meta.cur[0]), meta.scale[0].double())
    q, qt, db, cur, sc = out[True, True, True]
    assert torch.equal(u8(qt), u8(q).t())
    assert torch.equal(u8(out[True, False, True][0]), u8(q))
    assert torch.equal(u8(out[False, True, True][1]), u8(qt))
    assert torch.equal(u8(out[True, True, False][0]), u8(q)) and torch.equal(u8(out[True, True, False][1]), u8(qt))
    _check_codes(f"gelu bwd {case.R}x{case.C} fmt{fmt}", q, ref_quant(case.vb * sc, fmt), fmt)
    tol = MARGIN * case.e_amax_b                            # e_amax_b ~3e-7 at these shapes
    print(f"gelu bwd {case.R}x{case.C}: amax rel err {abs(cur - case.amax_b) / case.amax_b:.3e} (tol {tol:.3e})")
    assert abs(cur - case.amax_b) <= tol * case.amax_b
    assert all(o[3] == cur for o in out.values())
    # dbias, every column: bf16 output rounding + fp32 accumulation of R terms + formula error (e_col ~2.5e-7)
    bound = 2.0 ** -8 * case.db_ref.abs() + (case.R * 2.0 ** -24 + MARGIN * case.e_col) * case.db_S
    for key, o in out.items():
        if key[2]:
            assert o[2].shape == (case.C,) and o[2].dtype == BF16
            err = (o[2].double() - case.db_ref).abs()
            assert bool((err <= bound).all()), (key, float((err / bound).max()))
            assert torch.equal(o[2], db)                    # the same partial sums in every form


@pytest.mark.gpu
def test_bias_gelu_cast_transpose_vs_float64(gelu_case):
    _gelu_fwd(gelu_case, 0)
    if (gelu_case.R, gelu_case.C) in ((192, 320), (256, 384)):
        _gelu_fwd(gelu_case, 1)                             # the other format, once per tile kernel


@pytest.mark.gpu
def test_bias_gelu_bwd_cast_transpose_vs_float64(gelu_case):
    _gelu_bwd(gelu_case, 1)
    if (gelu_case.R, gelu_case.C) in ((192, 320), (256, 384)):
        _gelu_bwd(gelu_case, 0)


# ---------------------------------------------------------------------------------------------------------------
# 5. device scale update against the CPU path
# ---------------------------------------------------------------------------------------------------------------

def _amax_sequence(H):
    """Per-step amax of one slot: a rising value, a large one that later leaves the H-deep window, +inf (old scale
    kept, the inf stays in the history until it rolls out), a denormal-small positive value and zeros."""
    seq = [1.5, 2.0, 3.0, 1e30] + [4.0 + 0.25 * i for i in range(H + 1)]
    seq += [float("inf")] + [0.5 + 0.125 * i for i in range(H + 1)]
    seq += [1e-40] + [0.0] * (H + 1) + [6.0]
    return seq


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("s0,s1", [(0, 2), (2, 3), (0, 3)])
@pytest.mark.parametrize("margin", [0, 2])
@pytest.mark.parametrize("H", [1, 4, 16])
def test_update_scales_device_matches_cpu(H, margin, s0, s1, fmt):
    g, c = F8.Fp8Meta("cuda", history=H, margin=margin), F8.Fp8Meta("cpu", history=H, margin=margin)
    outside = [s for s in range(3) if not s0 <= s < s1]
    for m in (g, c):                                        # sentinels in the slots the update must not touch
        for s in outside:
            m.hist[s] = 7.0 + s
            m.cur[s] = 3.25
            m.scale[s] = 5.0
            m.scale_inv[s] = 0.2
    names = ("hist", "cur", "scale", "scale_inv")
    before = {n: getattr(c, n).clone() for n in names}
    seq = _amax_sequence(H)
    for step, v in enumerate(seq):
        for s in range(s0, s1):
            # slot s0 starts with amax 0 (scale and scale_inv must stay 1); the slots differ by a factor
            val = 0.0 if (step == 0 and s == s0) else v * (1.0 + 0.5 * (s - s0))
            g.cur[s] = val
            c.cur[s] = val
        old_scale = c.scale.clone()
        g.update(s0, s1, fmt)
        c.update(s0, s1, fmt)
        got = {n: getattr(g, n).cpu() for n in names}
        # exact: both sides are IEEE fp32 divisions, no fast-math.  (Fp8Meta.update's CPU path must divide tensor by
        # tensor: ``float / tensor`` is reciprocal-then-multiply in torch and was one ulp off the kernel.)
        for n in ("hist", "scale", "scale_inv"):
            assert torch.equal(got[n], getattr(c, n)), (step, n, got[n], getattr(c, n))
        assert bool((got["cur"][s0:s1] == 0).all())
        for n in names:
            for s in outside:
                assert torch.equal(got[n][s], before[n][s]), (step, n, s)
        # the CPU side itself does what the recipe says
        if step == 0:
            assert float(c.scale[s0]) == 1.0 and float(c.scale_inv[s0]) == 1.0
        if v == float("inf"):
            assert torch.equal(c.scale[s0:s1], old_scale[s0:s1]) and bool(torch.isinf(c.hist[s0:s1, 0]).all())
    assert bool(torch.isfinite(c.hist[s0:s1]).all())        # the inf rolled out
    assert float(c.scale[s0]) == float(torch.tensor(FMT_MAX[fmt]) / torch.tensor(6.0) * 2.0 ** -margin)
