"""The row-wise checker (tests/rowwise_ref.py) has teeth, shown without a GPU.  For every case the GPU suite runs:
(a) an honest float32 torch evaluation of the same formula, rounded to the output dtype, scores <= 0.5, so the
GPU test (threshold 1) cannot fail an honest kernel for its rounding alone; (b) each of a list of subtly wrong
float32 evaluations -- the mistakes the first-generation whole-tensor metric let through -- is rejected by at
least one case."""
import math

import pytest
import torch

import rowwise_ref as R
from rowwise_ref import BF16, F32, f64

HONEST = 0.5


def _scores(pairs, limit=HONEST):
    """pairs: (name, got, (ref, mag), out_dtype).  Asserts every one under `limit`, returns the maxima."""
    return {name: R.check(name, got, ref, mag, dt, limit) for name, got, (ref, mag), dt in pairs}


def _any_rejected(pairs):
    return any(R.rejected(got, ref, mag, dt) for _, got, (ref, mag), dt in pairs)


# ---------------------------------------------------------------------------------------------------------------
# the checker itself
# ---------------------------------------------------------------------------------------------------------------

def test_ulp_bf16_is_the_bf16_spacing():
    v = torch.tensor([1.0, 1.0 - 2.0 ** -8, 1.5, 2.0, -3.0, 1.5 * 2.0 ** -10, 304.0, 2.0 ** -126, 0.0, 1e-45],
                     dtype=torch.float64)                              # all bf16 values, so the binade is theirs
    want = []
    for x in v.tolist():
        b = torch.tensor([abs(x)], dtype=torch.float32).to(BF16)
        if float(b) < 2.0 ** -126:
            want.append(2.0 ** -133)
            continue
        down = (b.view(torch.int16) & 0x7F80).view(BF16)           # the binade's power of two
        want.append(float(down.double()) * 2.0 ** -7)
    assert R.ulp_bf16(v).tolist() == want


def test_checker_reports_the_worst_element():
    ref = torch.zeros(3, 4, dtype=torch.float64)
    mag = torch.ones(3, 4, dtype=torch.float64)
    got = torch.zeros(3, 4)
    assert R.check("zeros", got, ref, mag, F32) == 0.0
    got[2, 1] = 3.0 * R.REL
    with pytest.raises(AssertionError, match=r"row 2, col 1.*got 2.86\d+e-06, ref 0.0"):
        R.check("one off", got, ref, mag, F32)
    got[2, 1] = float("nan")
    with pytest.raises(AssertionError, match="scaled error inf"):
        R.check("nan", got, ref, mag, F32)
    # an exact result passes even where the allowance is zero; anything else does not
    assert R.check("exact", torch.zeros(2), torch.zeros(2, dtype=torch.float64), torch.zeros(2), F32) == 0.0
    assert R.rejected(torch.tensor([1e-30]), torch.zeros(1, dtype=torch.float64), torch.zeros(1), F32)
    # bf16: exactly half an ulp (a correctly rounded tie) scores 0.5
    assert R.check("tie", torch.tensor([1.0]), torch.tensor([1.0 + 2.0 ** -8], dtype=torch.float64),
                   torch.zeros(1), BF16) == 0.5


# ---------------------------------------------------------------------------------------------------------------
# norms
# ---------------------------------------------------------------------------------------------------------------

def norm_fwd_f32(c, xn, w, b, mutant=None):
    x, w = xn.float(), w.float().view(1, -1)
    N = x.shape[1]
    mean = torch.zeros(x.shape[0], 1) if c.rms else x.sum(1, keepdim=True) / N
    d = x if (c.rms or mutant == "no_mean") else x - mean
    var = (d * d).sum(1, keepdim=True) / (N - 1 if mutant == "nm1" else N)
    rstd = torch.rsqrt(var + (0.0 if mutant == "no_eps" else R.NORM_EPS))
    ry = rstd
    if mutant == "prev_rstd" and x.shape[0] > 1:
        ry = rstd.clone()
        ry[-1] = rstd[-2]
    y = d * ry * w
    if b is not None:
        y = y + b.float().view(1, -1)
    return y.to(c.xdt), mean, rstd


def norm_bwd_f32(c, d, e, mutant=None):
    x, dy, w = e["xn"].float(), d["dy"].float(), d["w"].float().view(1, -1)
    N = x.shape[1]
    mean, rstd = e["mean32"], e["rstd32"]
    xh = (x - mean) * rstd
    g = dy * w
    c1 = (g * xh).sum(1, keepdim=True) / N
    c2 = 0.0 if c.rms else g.sum(1, keepdim=True) / N
    dx = rstd * (g - c2 - xh * c1)
    if c.dres and mutant != "no_dres":
        dx = dx + d["dres"].float()
    dxs = dx.to(c.xdt)
    keep = slice(None, -1) if mutant == "last_row_missing" else slice(None)
    dg, db, ds = (dy * xh)[keep].sum(0), dy[keep].sum(0), dxs.float()[keep].sum(0)
    if mutant == "col2x":
        dg[N // 2] *= 2.0
        db[N - 1] *= 2.0
    if c.acc and mutant != "no_acc":
        dg, db = dg + d["prev_dgamma"].float(), db + d["prev_dbeta"].float()
    return dxs, dg.to(c.wdt), db.to(c.wdt), ds.to(c.wdt)


def _norm_pairs(c, d, e, fwd_mut=None, bwd_mut=None):
    y, mean, rstd = norm_fwd_f32(c, e["xn"], d["w"], d["b"], fwd_mut)
    dx, dg, db, ds = norm_bwd_f32(c, d, e, bwd_mut)
    pairs = [("y", y, e["fwd"]["y"], c.xdt), ("rstd", rstd, e["fwd"]["rstd"], F32),
             ("dx", dx, e["bwd"]["dx"], c.xdt), ("dgamma", dg, e["bwd"]["dgamma"], c.wdt)]
    if not c.rms:
        pairs.append(("mean", mean, e["fwd"]["mean"], F32))
    if c.has_b:
        pairs.append(("dbeta", db, e["bwd"]["dbeta"], c.wdt))
    if c.ds:
        pairs.append(("ds", ds, e["bwd"]["ds"], c.wdt))
    if c.res:
        pairs.append(("s", e["s_stored"], e["s"], c.xdt))
    return pairs


@pytest.fixture(scope="module")
def norm_data():
    cache = {}

    def get(c):
        if c.idx not in cache:
            d = R.norm_inputs(c)
            cache[c.idx] = (d, R.norm_expected(c, d))
        return cache[c.idx]
    return get


@pytest.mark.parametrize("c", R.NORM_CASES, ids=R.norm_id)
def test_norm_honest_float32_scores_under_half(c, norm_data):
    d, e = norm_data(c)
    _scores(_norm_pairs(c, d, e))


def test_norm_case_list_covers_the_recipe():
    cs = R.NORM_CASES
    assert {c.N for c in cs} == set(R.NORM_WIDTHS) | {5464}
    for N in R.NORM_WIDTHS:
        mine = [c for c in cs if c.N == N]
        assert {c.rows for c in mine} >= {1, 19} and {c.flags for c in mine} == {f[0] for f in R.NORM_FLAGS}
    assert {(c.xdt, c.wdt) for c in cs} == {(a, b) for a in (BF16, F32) for b in (BF16, F32)}
    assert {(c.N, c.ds) for c in cs if c.N == 5464} == {(5464, False), (5464, True)}
    d = R.norm_inputs(next(c for c in cs if c.rows == 19 and not c.res))
    x = d["x"].float()
    assert bool((x[1] == 0).all()) and bool((x[2] == x[2, 0]).all()) and float(d["w"][0]) == 0 and float(d["w"][1]) < 0


@pytest.mark.parametrize("mutant", ["no_mean", "nm1", "no_eps", "prev_rstd"])
def test_norm_forward_mutants_are_rejected(mutant, norm_data):
    for c in R.NORM_CASES:
        if c.N > 2056 or (mutant == "no_mean" and c.rms):
            continue
        d, e = norm_data(c)
        if _any_rejected(_norm_pairs(c, d, e, fwd_mut=mutant)):
            return
    pytest.fail(f"no case rejects the forward mutant {mutant}")


@pytest.mark.parametrize("mutant", ["col2x", "last_row_missing", "no_dres", "no_acc"])
def test_norm_backward_mutants_are_rejected(mutant, norm_data):
    for c in R.NORM_CASES:
        if c.N > 2056 or (mutant == "no_dres" and not c.dres) or (mutant == "no_acc" and not c.acc):
            continue
        d, e = norm_data(c)
        if _any_rejected(_norm_pairs(c, d, e, bwd_mut=mutant)):
            return
    pytest.fail(f"no case rejects the backward mutant {mutant}")


@pytest.mark.parametrize("mutant", ["no_mean", "nm1", "col2x"])
def test_norm_mutants_are_rejected_at_every_width(mutant, norm_data):
    """The mistakes that hide in a whole-tensor ratio (they scored 0.002 - 0.008 against limits of 0.01 - 0.02)
    are caught at EVERY width, the widest included, not just somewhere in the list."""
    for N in R.NORM_WIDTHS:
        hit = False
        for c in (c for c in R.NORM_CASES if c.N == N and c.rows > 1 and not (mutant == "no_mean" and c.rms)):
            d, e = norm_data(c)
            fm, bm = (None, mutant) if mutant == "col2x" else (mutant, None)
            hit = hit or _any_rejected(_norm_pairs(c, d, e, fwd_mut=fm, bwd_mut=bm))
        assert hit, f"N = {N}: {mutant} not rejected"


# ---------------------------------------------------------------------------------------------------------------
# bias + GELU
# ---------------------------------------------------------------------------------------------------------------

def _gelu_f32(u, tanh):
    if tanh:
        p = 2.0 * R.K0 * (u + R.KC * u * u * u)
        s = torch.sigmoid(p)
        q = 2.0 * R.K0 * (1.0 + 3.0 * R.KC * u * u)
        return u * s, s + u * (s * (1.0 - s)) * q
    cdf = 0.5 * (1.0 + torch.erf(u * (1.0 / math.sqrt(2.0))))
    return u * cdf, cdf + u * (torch.exp(-0.5 * u * u) * (1.0 / math.sqrt(2.0 * math.pi)))


def gelu_f32(c, d, with_bias=True, mutant=None):
    h, dy, b = d["h"].float(), d["dy"].float(), d["bias"].float()
    if mutant == "bias_vec0_last8":
        b = b.clone()
        b[-8:] = b[:8]
    u = h + b.view(1, -1) if with_bias else h
    tanh = c.tanh if mutant != "swap" else not c.tanh
    y, der = _gelu_f32(u, tanh)
    dh = dy * der
    keep = slice(None, -1) if mutant == "last_row_missing" else slice(None)
    db = dh[keep].sum(0)
    if mutant == "col2x":
        db[c.N // 2] *= 2.0
    if c.acc and mutant != "no_acc":
        db = db + d["prev_dbias"].float()
    return y.to(c.hdt), dh.to(c.hdt), db.to(c.bdt)


def _gelu_pairs(c, d, mutant=None, with_bias=True):
    hb = f64(d["bias"]) if with_bias else None
    y, dh, db = gelu_f32(c, d, with_bias, mutant)
    fr = R.bias_gelu_ref(f64(d["h"]), hb, c.tanh)
    br = R.bias_gelu_bwd_ref(f64(d["dy"]), f64(d["h"]), hb, 1 if c.tanh else 0,
                             f64(d["prev_dbias"]) if c.acc else None)
    pairs = [("y", y, fr["y"], c.hdt), ("dh", dh, br["dh"], c.hdt)]
    if with_bias:
        pairs.append(("dbias", db, br["dbias"], c.bdt))
    return pairs


@pytest.mark.parametrize("c", R.GELU_CASES + [R.GELU_TWO_PASS], ids=R.gelu_id)
def test_gelu_honest_float32_scores_under_half(c):
    d = R.gelu_inputs(c)
    _scores(_gelu_pairs(c, d))
    if c.rows <= 13:
        _scores(_gelu_pairs(c, d, with_bias=False))
        m2 = R.bias_gelu_bwd_ref(f64(d["dy"]), f64(d["hd"]), None, 2, f64(d["prev_dbias"]) if c.acc else None)
        dh = d["dy"].float() * d["hd"].float()
        db = dh.sum(0) + (d["prev_dbias"].float() if c.acc else 0.0)
        _scores([("dh2", dh.to(c.hdt), m2["dh"], c.hdt), ("dbias2", db.to(c.bdt), m2["dbias"], c.bdt)])


def test_gelu_case_list_covers_the_recipe():
    cs = R.GELU_CASES
    for N in R.GELU_WIDTHS:
        mine = [c for c in cs if c.N == N]
        assert [c.rows for c in mine] == R.GELU_ROWS
        assert {(c.hdt, c.bdt) for c in mine} == set(R.GELU_DTYPES) and {c.tanh for c in mine} == {True, False}
        assert {c.acc for c in mine} == {0, 1}
    c = next(c for c in cs if c.N == 2048 and c.rows == 5)
    d = R.gelu_inputs(c)
    u = (d["h"].float() + d["bias"].float().view(1, -1))[0, :12]
    assert torch.equal(u, torch.tensor(R.GELU_PLANTED).to(c.hdt).float())      # planted values survive the bias
    assert R.GELU_TWO_PASS.rows * R.GELU_TWO_PASS.N // 8 > 4096 * 256 and (4096 * 256 * 8) % R.GELU_TWO_PASS.N == 128


@pytest.mark.parametrize("mutant", ["bias_vec0_last8", "swap", "col2x", "last_row_missing", "no_acc"])
def test_gelu_mutants_are_rejected(mutant):
    hits = {True: False, False: False}                       # "swap": erf for tanh AND tanh for erf, bf16 included
    for c in R.GELU_CASES:
        if (mutant == "no_acc" and not c.acc) or (mutant == "swap" and c.hdt != BF16):
            continue
        if _any_rejected(_gelu_pairs(c, R.gelu_inputs(c), mutant)):
            hits[c.tanh] = True
        if all(hits.values()):
            return
    pytest.fail(f"GELU mutant {mutant}: rejected for tanh / erf cases: {hits}")


def test_gelu_bias_mutant_is_rejected_at_every_width():
    for N in R.GELU_WIDTHS[1:]:                              # N = 8 has a single vector
        assert any(_any_rejected(_gelu_pairs(c, R.gelu_inputs(c), "bias_vec0_last8"))
                   for c in R.GELU_CASES if c.N == N), N


# ---------------------------------------------------------------------------------------------------------------
# SwiGLU
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", R.SWIGLU_CASES, ids=R.swiglu_id)
def test_swiglu_honest_float32_scores_under_half(c):
    d = R.swiglu_inputs(c)
    x, dy = d["x"].float(), d["dy"].float()
    a, b = x[:, :c.F], x[:, c.F:]
    s = torch.sigmoid(a)
    y = a * s * b
    dx = torch.cat([dy * b * (s + a * (s * (1.0 - s))), dy * a * s], 1)
    _scores([("y", y.to(c.dt), R.swiglu_ref(f64(d["x"]))["y"], c.dt),
             ("dx", dx.to(c.dt), R.swiglu_bwd_ref(f64(d["dy"]), f64(d["x"]))["dx"], c.dt)])
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all())
    # the wrong sign on the up-projection gradient, and gate / up exchanged, are rejected
    ref = R.swiglu_bwd_ref(f64(d["dy"]), f64(d["x"]))["dx"]
    assert R.rejected(torch.cat([dx[:, c.F:], dx[:, :c.F]], 1).to(c.dt), ref[0], ref[1], c.dt)


# ---------------------------------------------------------------------------------------------------------------
# RoPE
# ---------------------------------------------------------------------------------------------------------------

def rope_f32(c, x, cos, sin, inverse, mutant=None):
    """x [B, S, H, D] -> rotated, position by explicit index arithmetic so that the mutants can get it wrong."""
    B, S, H, D = x.shape
    h = D // 2
    s_idx = torch.arange(S).view(1, S, 1).expand(B, S, H)
    h_idx = torch.arange(H).view(1, 1, H).expand(B, S, H)
    pos = (h_idx if mutant == "head_for_pos" else s_idx) + (0 if mutant == "no_pos0" else c.pos0)
    if mutant == "pos_off1":
        pos = pos + 1
    cs, sn = cos[pos], sin[pos]                               # [B, S, H, D/2]
    if inverse and mutant != "no_sign_flip":
        sn = -sn
    a, b = x.float()[..., :h], x.float()[..., h:]
    return torch.cat([a * cs - b * sn, b * cs + a * sn], -1).to(c.dt)


@pytest.mark.parametrize("c", R.ROPE_CASES, ids=R.rope_id)
def test_rope_honest_float32_scores_under_half(c):
    d = R.rope_inputs(c)
    x = d["packed"][:, :, :c.H]
    cos64, sin64 = f64(d["cos"]), f64(d["sin"])
    for inv in (False, True):
        ref = R.rope_ref(f64(x), cos64, sin64, c.pos0, inv)["y"]
        _scores([("rope", rope_f32(c, x, d["cos"], d["sin"], inv), ref, c.dt)])
    fwd = rope_f32(c, x, d["cos"], d["sin"], False)
    back = rope_f32(c, fwd, d["cos"], d["sin"], True)
    yref = R.rope_ref(f64(x), cos64, sin64, c.pos0)["y"][0]
    _scores([("roundtrip", back, (f64(x), R.rope_roundtrip_mag(yref, cos64, sin64, c.pos0, c.dt)), c.dt)])


@pytest.mark.parametrize("mutant", ["pos_off1", "no_sign_flip", "no_pos0", "head_for_pos"])
def test_rope_mutants_are_rejected(mutant):
    n = 0
    for c in R.ROPE_CASES:
        if mutant == "no_pos0" and c.pos0 == 0:
            continue
        d = R.rope_inputs(c)
        x = d["packed"][:, :, :c.H]
        inv = mutant == "no_sign_flip"
        ref = R.rope_ref(f64(x), f64(d["cos"]), f64(d["sin"]), c.pos0, inv)["y"]
        assert R.rejected(rope_f32(c, x, d["cos"], d["sin"], inv, mutant), ref[0], ref[1], c.dt), R.rope_id(c)
        n += 1
    assert n >= len(R.ROPE_CASES) // 2


def test_rope_tables_are_fenced_with_nan():
    cos, sin = R.rope_tables(32, 7, R.ROPE_S)
    ok = torch.zeros(cos.shape[0], dtype=torch.bool)
    ok[7:7 + R.ROPE_S] = True
    assert bool(torch.isfinite(cos[ok]).all()) and bool(torch.isnan(cos[~ok]).all()) and bool(torch.isnan(sin[~ok]).all())
    assert all(c.H != R.ROPE_S for c in R.ROPE_CASES)


# ---------------------------------------------------------------------------------------------------------------
# cast inputs
# ---------------------------------------------------------------------------------------------------------------

def test_cast_inputs_hold_what_they_claim():
    x, sub = R.cast_inputs(4099)
    assert x.numel() == 4099 and int(sub.sum()) == 10
    bits = x.view(torch.int32)
    assert int(torch.isnan(x).sum()) == 1 and int(torch.isinf(x).sum()) == 2
    assert int((bits == 0).sum()) >= 1 and int((bits == -2 ** 31).sum()) >= 1
    assert int(((bits & 0xFFFF) == 0x8000).sum()) >= 60                       # exact ties
    ties = x[((bits & 0xFFFF) == 0x8000) & torch.isfinite(x) & ~sub]
    lo = (ties.view(torch.int32) & -65536).view(F32)
    up = ties.to(BF16).float()
    even = (ties.view(torch.int32) >> 16) & 1                                  # parity of the lower neighbour
    assert bool(((up == lo) == (even == 0)).all()) and 0 < int(even.sum()) < ties.numel()
    assert [R.cast_inputs(n)[0].numel() for n in R.CAST_SIZES] == R.CAST_SIZES
