"""float64 references, error magnitudes, the per-element checker and the case lists for the row-wise kernels
(LayerNorm / RMSNorm, bias + GELU, SwiGLU, RoPE, the fp32 -> bf16 cast).  No GPU is needed to import this module;
tests/test_rowwise_ref_cpu.py proves on the CPU that the checker accepts an honest float32 evaluation and rejects
a list of subtly wrong ones, tests/test_rowwise_kernels_gpu.py applies the same cases to the HIP kernels.

The checker.  Every reference returns, next to each value, a *magnitude*: the float64 sum of the absolute values
of the intermediates that an fp32 evaluation rounds on its way to that element.  An output element passes when

    |got - ref|  <=  ulp_out(ref) + 2^-20 * magnitude

ulp_out is the bf16 spacing at ref for a bf16 output (rounding the exact value costs half of it; a value that
carries a small fp32 error in front of a tie can land on the other neighbour, which stays under one) and 0 for an
fp32 output.  2^-20 is 16 fp32 roundings of the full magnitude (fp32 eps = 2^-24 here, the half-ulp relative
error): every formula below rounds a handful of times, so an honest kernel sits well under 1 and the CPU
self-test demands <= 0.5 of an honest float32 evaluation.  Neither number is tuned to any kernel's result.

The references are written from the operations' definitions; they take the stored input values (bf16 upcast
exactly) so that input quantisation is not part of the error.
"""
import math
from collections import namedtuple

import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
REL = 2.0 ** -20
# An fp32 intermediate that underflows is flushed or rounded with an ABSOLUTE error of up to the smallest normal
# number 2^-126, not a relative one (the hardware exponential and reciprocal return 0 for a subnormal result).  Like
# every allowance here it is budgeted at twice the honest worst case: a magnitude term of 2^-105 turns into 2^-125.
FLOOR = 2.0 ** -105


# ---------------------------------------------------------------------------------------------------------------
# checker
# ---------------------------------------------------------------------------------------------------------------

def ulp_bf16(ref):
    """Spacing of bf16 at |ref| (float64 tensor): 2^(floor(log2 |ref|) - 7), and the subnormal spacing 2^-133
    below the smallest normal number (0 included)."""
    a = ref.abs()
    _, e = torch.frexp(a)                                  # a = m * 2^e, m in [0.5, 1)
    e = torch.where(a > 0, e, torch.full_like(e, -125)).clamp(min=-125)
    return torch.exp2(e.double() - 8.0)


def ulp_out(ref, out_dtype):
    return ulp_bf16(ref) if out_dtype == BF16 else torch.zeros_like(ref)


def scaled_error(got, ref, mag, out_dtype):
    """Per-element |got - ref| / (ulp_out(ref) + 2^-20 * mag) in float64.  An exact match scores 0 even where the
    allowance is 0; a non-finite `got` against a finite reference scores inf."""
    ref = ref.double()
    g = got.detach().cpu().double().reshape(ref.shape)
    mag = mag.double().expand_as(ref)
    err = (g - ref).abs()
    sc = err / (ulp_out(ref, out_dtype) + REL * mag)
    sc = torch.where(err == 0, torch.zeros_like(sc), sc)
    return torch.where(torch.isfinite(g) | ~torch.isfinite(ref), sc, torch.full_like(sc, float("inf")))


def check(name, got, ref, mag, out_dtype, limit=1.0):
    """Assert max(scaled) <= limit; returns the maximum.  The failure names the worst element."""
    sc = scaled_error(got, ref, mag, out_dtype)
    if sc.numel() == 0:
        return 0.0
    flat = sc.reshape(-1)
    flat = torch.where(torch.isnan(flat), torch.full_like(flat, float("inf")), flat)
    worst = float(flat.max())
    if not worst <= limit:
        i = int(flat.argmax())
        ncol = ref.shape[-1] if ref.dim() >= 1 else 1
        g = got.detach().cpu().double().reshape(-1)[i]
        raise AssertionError(
            f"{name}: scaled error {worst:.4g} > {limit} at flat index {i} (row {i // ncol}, col {i % ncol}): "
            f"got {float(g)!r}, ref {float(ref.double().reshape(-1)[i])!r}, "
            f"magnitude {float(mag.double().expand_as(ref).reshape(-1)[i]):.6g}")
    return worst


def rejected(got, ref, mag, out_dtype):
    """True when the checker would fail `got` (used by the mutant tests)."""
    sc = scaled_error(got, ref, mag, out_dtype)
    return bool((~(sc <= 1.0)).any())


def f64(t):
    return None if t is None else t.detach().cpu().double()


# ---------------------------------------------------------------------------------------------------------------
# LayerNorm / RMSNorm
# ---------------------------------------------------------------------------------------------------------------

def stored_sum(x, res, rb):
    """The fused residual sum as the kernels promise to store it: x + (res + res_bias) in fp32, in that order,
    rounded once to the activation dtype.  The norm is taken of these stored values."""
    r = res.float()
    if rb is not None:
        r = r + rb.float()
    return (x.float() + r).to(x.dtype)


def fused_sum_ref(x, res, rb):
    """float64 s = x + (res + res_bias) and its magnitude |x| + |res| + |res_bias| (two fp32 additions)."""
    s, m = x + res, x.abs() + res.abs()
    if rb is not None:
        s, m = s + rb, m + rb.abs()
    return s, m


def norm_fwd_ref(x, w, b, eps, rms):
    """x [rows, N] float64: the stored values being normalised; w, b [N] float64 (b None: no shift).
    Returns {name: (value, magnitude)} for y [rows, N], mean [rows, 1] (zeros for RMSNorm) and rstd [rows, 1].

    Magnitudes (eps32 = one fp32 rounding, A = mean_k |x_k|, d = x - mean, r = rstd):
      mean   an fp32 sum of N terms divided by N: the error is a few eps32 of sum |x_k| / N = A.
      rstd   r = (var + eps)^-1/2, dr/r = -dvar / (2 (var + eps)).  Every d_k carries the SAME mean error dm, and
             sum_k d_k = 0, so var only moves by dm^2 (second order) plus a few eps32 of var itself from the squares
             and the sum: dr <= r (c eps32 + dm^2 r^2 / 2).  With dm <= 4 eps32 A the second-order part is
             8 r (eps32 r A)^2 = 2^-20 * r * (r A)^2 * 2^-25: the factor k2 = 1 + 2^-25 (r A)^2 below.  It only
             matters for rows that are constant up to rounding (var << eps) around a large mean.
      y      (d r) w + b: d is rounded at |d| and inherits dm ~ eps32 A, r its own error, the product and the sum
             round once more: (|d| k2 + A) r |w| + |b|.  The A r |w| term is the conditioning of an off-centre row:
             the error of the mean is amplified by r whether or not the element itself is large.
      RMSNorm has no mean: r rounds at r (the mean square is a sum of positive terms), y at |x| r |w|.
    """
    w = w.view(1, -1)
    A = x.abs().mean(1, keepdim=True)
    if rms:
        mean = torch.zeros_like(A)
        r = ((x * x).mean(1, keepdim=True) + eps).rsqrt()
        y = x * r * w
        return {"y": (y, x.abs() * r * w.abs()), "mean": (mean, A), "rstd": (r, r)}
    mean = x.mean(1, keepdim=True)
    d = x - mean
    r = ((d * d).mean(1, keepdim=True) + eps).rsqrt()
    k2 = 1.0 + 2.0 ** -25 * (r * A) ** 2
    y = d * r * w
    mag = (d.abs() * k2 + A) * r * w.abs()
    if b is not None:
        y, mag = y + b.view(1, -1), mag + b.abs().view(1, -1)
    return {"y": (y, mag), "mean": (mean, A), "rstd": (r, r * k2)}


def norm_bwd_ref(dy, x, w, mean, rstd, dres, rms, act_dtype, prev_dgamma=None, prev_dbeta=None):
    """The backward of y = (x - mean) rstd w + b for given SAVED statistics: mean, rstd [rows, 1] are inputs (the
    fp32 values the forward stored, upcast), like x and dy.  dres (nullable) is added into dx.
    Returns {name: (value, magnitude)} for dx, dgamma, dbeta, ds (the column sum of dx).

      xh = (x - mean) rstd        one exact-or-half-ulp subtraction and one product: rounds at |xh|
      g  = dy w
      c1 = mean_k(g xh), c2 = mean_k(g)  (c2 = 0 for RMSNorm): fp32 sums, round at mean|g xh| and mean|g|
      dx = rstd (g - c2 - xh c1) + dres: the three terms round at their own size:
           rstd (|g| + mean|g| + |xh| mean|g xh|) + |dres|
      dgamma = sum_rows dy xh  -> sum_rows |dy xh|;   dbeta = sum_rows dy -> sum_rows |dy|  (+ |previous| when
           accumulating: the old value is one more term of the sum)
      ds = sum_rows dx.  The kernels sum dx AS STORED, so for a bf16 activation every term carries its storage
           rounding of up to half a bf16 ulp on top of its fp32 error.  Like every other allowance here it is
           budgeted at twice the honest worst case (the honest evaluation must stay under 0.5):
           sum_rows (mag_dx + 2^20 * ulp_bf16(dx)), the second part written as a magnitude so that 2^-20 of it is
           one ulp.  (The GPU test also checks ds against the sum of the dx the kernel stored, without this term.)
    """
    w = w.view(1, -1)
    d = x if rms else x - mean
    xh = d * rstd
    g = dy * w
    c1 = (g * xh).mean(1, keepdim=True)
    m1 = (g * xh).abs().mean(1, keepdim=True)
    if rms:
        c2 = m2 = torch.zeros_like(c1)
    else:
        c2, m2 = g.mean(1, keepdim=True), g.abs().mean(1, keepdim=True)
    dx = rstd * (g - c2 - xh * c1)
    mag_dx = rstd * (g.abs() + m2 + xh.abs() * m1)
    if dres is not None:
        dx, mag_dx = dx + dres, mag_dx + dres.abs()
    dgamma, mag_dg = (dy * xh).sum(0), (dy * xh).abs().sum(0)
    dbeta, mag_db = dy.sum(0), dy.abs().sum(0)
    if prev_dgamma is not None:
        dgamma, mag_dg = dgamma + prev_dgamma, mag_dg + prev_dgamma.abs()
    if prev_dbeta is not None:
        dbeta, mag_db = dbeta + prev_dbeta, mag_db + prev_dbeta.abs()
    mag_ds = mag_dx.sum(0)
    if act_dtype == BF16:
        mag_ds = mag_ds + (ulp_bf16(dx) / REL).sum(0)
    return {"dx": (dx, mag_dx), "dgamma": (dgamma, mag_dg), "dbeta": (dbeta, mag_db), "ds": (dx.sum(0), mag_ds)}


# ---------------------------------------------------------------------------------------------------------------
# bias + GELU
# ---------------------------------------------------------------------------------------------------------------

K0 = math.sqrt(2.0 / math.pi)
KC = 0.044715


def gelu_ref(u, tanh, u_is_sum=False):
    """GELU value y, derivative d and their magnitudes at the float64 pre-activation u.  Returns (y, my, d, md).

    tanh form: y = u/2 (1 + tanh z), z = K0 (u + KC u^3).  The definition cancels catastrophically for u << 0
    (1 + tanh z -> 0), so it is evaluated through the identity (1 + tanh z) / 2 = sigmoid(2 z), which has no
    cancellation; with p = 2 z, s = sigmoid(p), t = s (1 - s), q = dp/du = 2 K0 (1 + 3 KC u^2):
        y = u s,   d = s + u t q
      s    an fp32 evaluation computes exp(-p) from a ROUNDED exponent argument: the argument's error eps32 |p|
           becomes a relative error of the exponential, ds = s (1 - s) |p| eps32, next to the rounding of s
           itself -- ms = s + t |p|.  This is the term that grows with the exponent's argument and it alone
           limits the tail (|p| is 76 at u = -9.5).  Once exp(-p) leaves the fp32 range s is flushed: + FLOOR.
      y    |u| ms
      d    ms + |u| q (|1 - 2 s| ms + 2 t):  d(t) = (1 - 2 s) ds, and t and the product round at t.
    erf form: y = u Phi(u), Phi = (1 + erf(u / sqrt 2)) / 2, d = Phi + u phi(u), phi the normal density.  Here the
    definition itself is what fp32 evaluates, cancellation included, so the magnitude carries it: the sum
    1 + erf rounds at 1 + |erf|, and the rounded argument u / sqrt 2 moves erf by 2 |u| phi eps32:
        mPhi = (1 + |erf|) / 2 + |u| phi,  y: |u| mPhi
      phi  = exp(-u^2 / 2) / sqrt(2 pi) has the exponent argument u^2 / 2: mphi = phi (1 + u^2 / 2) + FLOOR
      d    mPhi + |u| mphi
    (Phi itself is taken from erfc, which is accurate in the tail.)
    u_is_sum: u was itself rounded (the kernel adds h + bias in fp32): + |u| |d| on y and + |u| |d'| on d.
    """
    au = u.abs()
    if tanh:
        p = 2.0 * K0 * (u + KC * u ** 3)
        s, s1 = torch.sigmoid(p), torch.sigmoid(-p)                    # s1 = 1 - s without cancellation
        t = s * s1
        q = 2.0 * K0 * (1.0 + 3.0 * KC * u * u)
        ms = s + t * p.abs() + FLOOR
        y, my = u * s, au * ms
        d = s + u * t * q
        md = ms + au * q * ((s1 - s).abs() * ms + 2.0 * t)
        d2 = 2.0 * t * q + u * q * q * t * (s1 - s) + u * t * (12.0 * K0 * KC * u)
    else:
        xr = u / math.sqrt(2.0)
        Phi = 0.5 * torch.special.erfc(-xr)
        phi = torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
        mPhi = 0.5 * (1.0 + torch.erf(xr).abs()) + au * phi
        mphi = phi * (1.0 + 0.5 * u * u) + FLOOR
        y, my = u * Phi, au * mPhi
        d, md = Phi + u * phi, mPhi + au * mphi
        d2 = phi * (2.0 - u * u)
    if u_is_sum:
        my, md = my + au * d.abs(), md + au * d2.abs()
    return y, my, d, md


def bias_gelu_ref(h, bias, tanh):
    """{y: (value, magnitude)} of gelu(h + bias); bias [N] or None."""
    u = h if bias is None else h + bias.view(1, -1)
    y, my, _, _ = gelu_ref(u, tanh, bias is not None)
    return {"y": (y, my)}


def bias_gelu_bwd_ref(dy, h, bias, mode, prev_dbias=None):
    """dh = dy gelu'(h + bias) and dbias = sum_rows dh (+ previous).  mode 0 erf, 1 tanh, 2: h already holds the
    derivative (dh = dy h, no bias).  dh rounds at |dy| md, dbias sums the unrounded dh: sum_rows |dy| md."""
    if mode == 2:
        dh, mdh = dy * h, (dy * h).abs()
    else:
        u = h if bias is None else h + bias.view(1, -1)
        _, _, d, md = gelu_ref(u, mode == 1, bias is not None)
        dh, mdh = dy * d, dy.abs() * md
    db, mdb = dh.sum(0), mdh.sum(0)
    if prev_dbias is not None:
        db, mdb = db + prev_dbias, mdb + prev_dbias.abs()
    return {"dh": (dh, mdh), "dbias": (db, mdb)}


# ---------------------------------------------------------------------------------------------------------------
# SwiGLU
# ---------------------------------------------------------------------------------------------------------------

def _sig_mag(a):
    """s = sigmoid(a), t = s (1 - s), 1 - 2 s, and ms = s + t |a| + FLOOR: s rounds at itself, the rounded exponent
    argument a contributes t |a| (see gelu_ref), and an exponential outside the fp32 range flushes s."""
    s, s1 = torch.sigmoid(a), torch.sigmoid(-a)
    t = s * s1
    return s, t, s1 - s, s + t * a.abs() + FLOOR


def swiglu_ref(x):
    """x [rows, 2F] -> y = silu(gate) up, gate = x[:, :F], up = x[:, F:].  y rounds at |gate up| ms."""
    F = x.shape[1] // 2
    a, b = x[:, :F], x[:, F:]
    s, _, _, ms = _sig_mag(a)
    return {"y": (a * s * b, (a * b).abs() * ms)}


def swiglu_bwd_ref(dy, x):
    """dx [rows, 2F]: dgate = dy up (s + gate t), dup = dy gate s.
      dgate  |dy up| (ms + |gate| (|1 - 2 s| ms + 2 t))   (d(t) = (1 - 2 s) ds; t and the products round at t)
      dup    |dy gate| ms"""
    F = x.shape[1] // 2
    a, b = x[:, :F], x[:, F:]
    s, t, s12, ms = _sig_mag(a)
    da = dy * b * (s + a * t)
    mda = (dy * b).abs() * (ms + a.abs() * (s12.abs() * ms + 2.0 * t))
    db, mdb = dy * a * s, (dy * a).abs() * ms
    return {"dx": (torch.cat([da, db], 1), torch.cat([mda, mdb], 1))}


# ---------------------------------------------------------------------------------------------------------------
# RoPE (rotate-half)
# ---------------------------------------------------------------------------------------------------------------

def rope_ref(x, cos, sin, pos0, inverse=False):
    """x [B, S, H, D] float64; cos, sin [S_max, D/2] float64 (the stored fp32 table values).  Position s of the
    sequence uses table row pos0 + s for every batch entry and head.
        out[..., i] = x[i] c - x[i + D/2] sn,  out[..., i + D/2] = x[i + D/2] c + x[i] sn   (inverse: sn -> -sn)
    Each output is a two-term fp32 sum of products: it rounds at |x[i] c| + |x[i + D/2] sn| (and the mirror)."""
    B, S, H, D = x.shape
    h = D // 2
    c = cos[pos0:pos0 + S].view(1, S, 1, h)
    sn = sin[pos0:pos0 + S].view(1, S, 1, h) * (-1.0 if inverse else 1.0)
    a, b = x[..., :h], x[..., h:]
    o = torch.cat([a * c - b * sn, b * c + a * sn], -1)
    m = torch.cat([(a * c).abs() + (b * sn).abs(), (b * c).abs() + (a * sn).abs()], -1)
    return {"y": (o, m)}


def rope_roundtrip_mag(y, cos, sin, pos0, act_dtype):
    """Magnitude for inverse(forward(x)) == x, given the float64 forward result y: the inverse rounds at
    |y1 c| + |y2 sn| as above, and for a bf16 activation its inputs are the STORED forward outputs, each off by up
    to half a bf16 ulp, which the rotation carries through with weights |c| and |sn|.  Budgeted at one ulp, twice
    the honest worst case like every allowance here, and written as a magnitude (2^-20 of it is the ulp)."""
    B, S, H, D = y.shape
    h = D // 2
    c = cos[pos0:pos0 + S].view(1, S, 1, h).abs()
    sn = sin[pos0:pos0 + S].view(1, S, 1, h).abs()
    a, b = y[..., :h].abs(), y[..., h:].abs()
    m = torch.cat([a * c + b * sn, b * c + a * sn], -1)
    if act_dtype == BF16:
        ua, ub = ulp_bf16(y[..., :h]) / REL, ulp_bf16(y[..., h:]) / REL
        m = m + torch.cat([ua * c + ub * sn, ub * c + ua * sn], -1)
    return m


def rope_tables(D, pos0, S, theta=10000.0):
    """cos / sin tables [pos0 + S + 2, D/2], built in float64 and stored as fp32; every row outside
    [pos0, pos0 + S) is NaN, so a wrong position poisons the output."""
    n = pos0 + S + 2
    inv = theta ** (-torch.arange(0, D // 2, dtype=F64) * 2.0 / D)
    ang = torch.arange(n, dtype=F64).view(-1, 1) * inv.view(1, -1)
    cos, sin = torch.cos(ang).float(), torch.sin(ang).float()
    bad = torch.ones(n, dtype=torch.bool)
    bad[pos0:pos0 + S] = False
    cos[bad] = float("nan")
    sin[bad] = float("nan")
    return cos, sin


# ---------------------------------------------------------------------------------------------------------------
# case lists and data recipes (shared by the CPU self-test and the GPU test)
# ---------------------------------------------------------------------------------------------------------------

def _gen(*key):
    g = torch.Generator()
    g.manual_seed(int(key[0]) * 1000003 + int(key[1]))
    return g


def _store(t32, dt):
    """Generated in fp32, rounded to the storage dtype; the reference sees the rounded values."""
    return t32.to(dt).contiguous()


NormCase = namedtuple("NormCase", "N rows flags xdt wdt rms has_b res rb dres ds acc idx")
# flag sets: every value of every flag occurs in one of them, and every width runs all four
#            name  x     w     rms    b      res    rb     dres   ds     accumulate
NORM_FLAGS = [
    ("plain", BF16, BF16, False, True, False, False, False, False, 0),   # LayerNorm, affine, packed dgamma + dbeta
    ("rmsfused", BF16, F32, True, False, True, True, True, True, 1),     # ds without db: the unpacked reduction
    ("nobias", F32, F32, False, False, True, False, True, False, 0),     # b null: the db == nullptr partial layout
    ("lnfused", F32, BF16, False, True, True, True, False, True, 1),     # ds with db: the packed 3-way reduction
]
NORM_EPS = 1e-5
# widths per dispatch branch of launch_fwd / launch_bwd (see the table in test_rowwise_kernels_gpu.py)
NORM_WIDTHS = [4, 60, 64, 68, 72, 100, 520, 2048, 2056, 2080, 4104, 4128, 8192, 8200, 8224, 16384, 16416]
NORM_WIDTHS_131 = [60, 100, 520, 2080]     # one width per kernel also gets rows = 131


def _norm_cases():
    out = []

    def add(N, rows, f):
        out.append(NormCase(N, rows, *NORM_FLAGS[f], len(out)))
    for i, N in enumerate(NORM_WIDTHS):        # rows = 1 and rows = 19 share the four flag sets, alternating by width
        one = (0, 3) if i % 2 == 0 else (1, 2)
        for f in range(4):
            add(N, 1 if f in one else 19, f)
    for N in NORM_WIDTHS_131:
        for f in range(4):
            add(N, 131, f)
    # the wave-per-row backward asks for (2 or 3) * N * 4 bytes of dynamic LDS: with ds that is 65,568 bytes here,
    # just past 64 KiB (N % 32 != 0 keeps the width off the row-split kernel)
    add(5464, 5, 0)
    add(5464, 5, 1)
    return out


NORM_CASES = _norm_cases()


def norm_id(c):
    return f"N{c.N}-r{c.rows}-{c.flags}"


NORM_MEANS = (0.0, 8.0, -8.0, 50.0)
NORM_STDS = (0.05, 1.0, 20.0)


def norm_inputs(c):
    """CPU tensors in their storage dtypes.  Per-row mean from {0, +-8, 50} and std from {0.05, 1, 20} (12 distinct
    pairs over 12 rows; a single-row case picks its pair by case index); row 1 all zero and row 2 constant when
    there are at least 3 rows; weights with an exact 0 and a negative entry; N(0, 1) gradients."""
    g = _gen(1, c.idx)
    rows, N = c.rows, c.N
    r = torch.arange(rows) + c.idx
    mean = torch.tensor(NORM_MEANS)[r % 4].view(-1, 1)
    std = torch.tensor(NORM_STDS)[r % 3].view(-1, 1)
    x = torch.randn(rows, N, generator=g) * std + mean
    res = torch.randn(rows, N, generator=g) * std if c.res else None
    if rows >= 3:
        x[1] = 0.0
        x[2] = 8.0
        if res is not None:
            res[1] = 0.0
            res[2] = 0.0
    w = torch.randn(N, generator=g)
    w[0] = 0.0
    w[1] = -0.5 - w[1].abs()
    d = {"x": _store(x, c.xdt), "w": _store(w, c.wdt),
         "b": _store(torch.randn(N, generator=g), c.wdt) if c.has_b else None,
         "res": _store(res, c.xdt) if c.res else None,
         "rb": _store(torch.randn(N, generator=g) * 0.5, c.wdt) if c.rb else None,
         "dy": _store(torch.randn(rows, N, generator=g), c.xdt),
         "dres": _store(torch.randn(rows, N, generator=g), c.xdt) if c.dres else None,
         "prev_dgamma": _store(torch.randn(N, generator=g) * 3.0, c.wdt),
         "prev_dbeta": _store(torch.randn(N, generator=g) * 3.0, c.wdt)}
    return d


def norm_expected(c, d):
    """Everything both tests compare against, computed once per case from the stored inputs:
    s_stored (None when not fused), fwd {y, mean, rstd}, the saved fp32 statistics fed to the backward, and
    bwd {dx, dgamma, dbeta, ds}."""
    s_st = stored_sum(d["x"], d["res"], d["rb"]) if c.res else None
    xn = s_st if c.res else d["x"]
    fwd = norm_fwd_ref(f64(xn), f64(d["w"]), f64(d["b"]), NORM_EPS, c.rms)
    mean32, rstd32 = fwd["mean"][0].float(), fwd["rstd"][0].float()
    acc = c.acc == 1
    bwd = norm_bwd_ref(f64(d["dy"]), f64(xn), f64(d["w"]), f64(mean32), f64(rstd32), f64(d["dres"]), c.rms, c.xdt,
                       f64(d["prev_dgamma"]) if acc else None, f64(d["prev_dbeta"]) if acc else None)
    fused = fused_sum_ref(f64(d["x"]), f64(d["res"]), f64(d["rb"])) if c.res else None
    return {"s_stored": s_st, "s": fused, "xn": xn, "fwd": fwd, "mean32": mean32, "rstd32": rstd32, "bwd": bwd}


GeluCase = namedtuple("GeluCase", "N rows tanh hdt bdt acc idx")
GELU_WIDTHS = [8, 120, 2040, 2048, 2056, 4104]     # < 2048: the row-packed kernel; >= 2048: the column-group kernel
GELU_ROWS = [1, 5, 6, 7, 9, 13, 131]
GELU_DTYPES = [(BF16, BF16), (BF16, F32), (F32, F32), (F32, BF16)]
# rows = 4100 at N = 2056: the smallest shape whose element-wise forward / backward takes a second grid-stride pass
# (4096 workgroups x 256 threads x 8 columns per pass) with a non-zero bias-column increment, (2^23 mod 2056) = 128
GELU_TWO_PASS = GeluCase(2056, 4100, True, BF16, F32, 0, 1000)
GELU_PLANTED = [0.0, -0.0, 9.5, -9.5, 10.2, -10.2, 12.0, -12.0, 40.0, -40.0, 1e4, -1e4]


def _gelu_cases():
    out = []
    for N in GELU_WIDTHS:
        for rows in GELU_ROWS:
            i = len(out)
            hdt, bdt = GELU_DTYPES[i % 4]
            out.append(GeluCase(N, rows, (i // 4 + i) % 2 == 0, hdt, bdt, (i // 2) % 2, i))
    return out


GELU_CASES = _gelu_cases()


def gelu_id(c):
    n = {BF16: "bf16", F32: "f32"}
    return f"N{c.N}-r{c.rows}-{'tanh' if c.tanh else 'erf'}-{n[c.hdt]}-{n[c.bdt]}-acc{c.acc}"


def gelu_planted_positions(c):
    """(row, col, value) of the planted pre-activations: the first min(N - 2, 12) columns, row after row, as far
    as the rows go.  The bias is 0 in those columns so that h + bias is the planted value itself."""
    ncol = min(c.N - 2, len(GELU_PLANTED))
    pos = [(k // ncol, k % ncol, v) for k, v in enumerate(GELU_PLANTED)]
    return ncol, [(r, col, v) for r, col, v in pos if r < c.rows]


def gelu_inputs(c):
    """h = 3 randn with the planted points; bias randn (0 under the planted columns); dy N(0, 1), exactly 1 at the
    planted points so that dh there is the derivative itself; hd: a stand-in derivative for mode 2."""
    g = _gen(2, c.idx)
    h = 3.0 * torch.randn(c.rows, c.N, generator=g)
    dy = torch.randn(c.rows, c.N, generator=g)
    bias = torch.randn(c.N, generator=g)
    ncol, pos = gelu_planted_positions(c)
    bias[:ncol] = 0.0
    for r, col, v in pos:
        h[r, col] = v
        dy[r, col] = 1.0
    return {"h": _store(h, c.hdt), "dy": _store(dy, c.hdt), "bias": _store(bias, c.bdt),
            "hd": _store(torch.randn(c.rows, c.N, generator=g) * 0.6 + 0.5, c.hdt),
            "prev_dbias": _store(torch.randn(c.N, generator=g) * 3.0, c.bdt)}


SwigluCase = namedtuple("SwigluCase", "F rows dt idx")
SWIGLU_CASES = [SwigluCase(F, rows, dt, i) for i, (F, rows, dt) in enumerate(
    (F, rows, dt) for F in (8, 104, 2000) for rows in (1, 3, 129) for dt in (BF16, F32))]
SWIGLU_PLANTED = [100.0, -100.0, 1e4, -1e4]


def swiglu_id(c):
    return f"F{c.F}-r{c.rows}-{'bf16' if c.dt == BF16 else 'f32'}"


def swiglu_inputs(c):
    """x = 2 randn [rows, 2F]; gate columns 0..3 of row 0 hold +-100 and +-1e4 (saturated sigmoid)."""
    g = _gen(3, c.idx)
    x = 2.0 * torch.randn(c.rows, 2 * c.F, generator=g)
    for k, v in enumerate(SWIGLU_PLANTED):
        x[0, k] = v
    return {"x": _store(x, c.dt), "dy": _store(torch.randn(c.rows, c.F, generator=g), c.dt)}


RopeCase = namedtuple("RopeCase", "D H pos0 dt idx")
ROPE_B, ROPE_S = 2, 5                                     # H is 1 or 3, never S: a head / position mix-up shows
ROPE_CASES = [RopeCase(D, H, p, dt, i) for i, (D, H, p, dt) in enumerate(
    (D, H, p, dt) for D in (16, 32, 64, 128) for H in (1, 3) for p in (0, 7) for dt in (BF16, F32))]
ROPE_LAYOUTS = ("contiguous", "packed_inplace", "packed_to_contiguous")


def rope_id(c):
    return f"D{c.D}-H{c.H}-pos{c.pos0}-{'bf16' if c.dt == BF16 else 'f32'}"


def rope_inputs(c):
    """packed [B, S, H + 2, D] N(0, 1) values (the first H heads are the ones rotated) and the NaN-fenced tables."""
    g = _gen(4, c.idx)
    packed = _store(torch.randn(ROPE_B, ROPE_S, c.H + 2, c.D, generator=g), c.dt)
    cos, sin = rope_tables(c.D, c.pos0, ROPE_S)
    return {"packed": packed, "cos": cos, "sin": sin}


CAST_SIZES = [1, 7, 8, 9, 4099]


def cast_inputs(n):
    """fp32 values for the cast: specials first (so that n = 1 .. 9 still see some), then exact ties between
    neighbouring bf16 values (both parities), then random values over many binades.  Returns (x, is_subnormal)."""
    g = _gen(5, n)
    big = torch.tensor([0x7F7FFFFF], dtype=torch.int32).view(F32)           # largest finite fp32
    sub = torch.tensor([0x00000001, 0x007FFFFF, 0x00400000, 0x00008000, 0x00018000], dtype=torch.int32).view(F32)
    spec = torch.cat([torch.tensor([0.0, -0.0, float("inf"), -float("inf"), float("nan")]), big, -big, sub, -sub])
    base = (torch.randn(64, generator=g) * 37.0).to(BF16).float()
    ties = (base.view(torch.int32) | 0x8000).view(F32)                      # exactly half way to the next bf16
    rnd = torch.randn(n, generator=g) * torch.exp2(torch.randint(-40, 40, (n,), generator=g).float())
    x = torch.cat([spec, ties, rnd])
    x = torch.roll(x, -(n % 5))[:n].contiguous() if n < 16 else x[:n].contiguous()
    bits = x.view(torch.int32) & 0x7FFFFFFF
    return x, (bits > 0) & (bits < 0x00800000)
