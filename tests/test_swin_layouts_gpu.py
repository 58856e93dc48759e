"""SwinIR's head-major attention path: every layout flag of the window-attention kernels and every dispatch /
fallback route of the projections around them, against fp64 references (MI355X).

The head-major tensors keep their token-major SHAPE; only the Python attribute ``_pdt_head_major`` says how the buffer
is laid out.  A wrong flag gives no fault and no shape error -- only wrong numbers -- so every case here compares
with an independent fp64 computation and asserts, through spies, which path it took.

Part A drives ``_WindowAttnFn`` / ``_WindowAttnTableFn`` directly (small window counts); part B a real
``SwinTransformerBlock`` at >= 16,384 tokens (the narrow GEMM's range) against a CPU fp64 copy of the block.
"""
import contextlib
import copy
import functools
import math
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def _tag(t):
    return getattr(t, "_pdt_head_major", None)


def _to_hm(t, N, parts, d):
    """[Bw, N, parts * d] token-major -> the same shape with the buffer [Bw, parts, N, d] (plain torch)."""
    Bw = t.shape[0]
    return t.reshape(Bw, N, parts, d).permute(0, 2, 1, 3).contiguous().view(Bw, N, parts * d)


def _from_hm(t, N, parts, d):
    Bw = t.shape[0]
    return t.reshape(Bw, parts, N, d).permute(0, 2, 1, 3).reshape(Bw, N, parts * d)


def _report(label, rows):
    """rows: (name, error, bound).  Every figure is printed before anything is asserted."""
    bad = []
    for name, err, bound in rows:
        print(f"{label} {name}: rel_err {err:.3e} (bound {bound:g})")
        if not err < bound:
            bad.append((name, err, bound))
    assert not bad, (label, bad)


def _same(label, got, want):
    """Layout only changes addresses: the same arithmetic on the same values (the block test's bounds)."""
    bad = []
    for k, v in want.items():
        g = got[k]
        if v is None or g is None:
            assert v is None and g is None, (label, k)
            continue
        diff = (g.double() - v.double()).abs().max().item()
        print(f"{label} {k}: max abs difference from the token-major run {diff:.3e}")
        try:
            torch.testing.assert_close(g, v, rtol=1e-5, atol=1e-6)
        except AssertionError as e:
            bad.append((k, str(e).splitlines()[:4]))
    assert not bad, (label, bad)


@pytest.fixture
def spies(monkeypatch):
    """Record the layout tags at the three hand-over points and the attention's own o_hm; narrow GEMM forced on
    (not this machine's timing pick)."""
    import pytorch_distributedtraining_amd.models.swinir as S
    import pytorch_distributedtraining_amd.ops.linear as L
    from pytorch_distributedtraining_amd.ops import window_attention as WA
    rec = SimpleNamespace(qkv=[], proj_in=[], do=[], o_hm=[], hm=[])
    real_fwd, real_bp, real_lfh = WA._WindowAttnFn.forward, WA._WindowAttnFn._backward_parts, L.linear_from_head_major

    def fwd(ctx, qkv, *a):
        rec.qkv.append(_tag(qkv))
        return real_fwd(ctx, qkv, *a)

    def bp(ctx, do):
        rec.do.append(_tag(do))
        rec.o_hm.append(ctx.o_hm)
        rec.hm.append(getattr(ctx, "hm", None))
        return real_bp(ctx, do)

    def lfh(module, x):
        rec.proj_in.append(_tag(x))
        return real_lfh(module, x)

    def clear():
        for v in vars(rec).values():
            if isinstance(v, list):
                v.clear()
    rec.clear = clear
    monkeypatch.setattr(WA._WindowAttnFn, "forward", staticmethod(fwd))
    monkeypatch.setattr(WA._WindowAttnFn, "_backward_parts", staticmethod(bp))
    monkeypatch.setattr(S, "linear_from_head_major", lfh)
    monkeypatch.setattr(L, "NARROW", "1")
    return rec


# ------------------------------------------------------------------------------------------------
# A. kernel layout matrix against fp64
# ------------------------------------------------------------------------------------------------
def _ref64(qkv, bias, mask, h, scale):
    """softmax(q k^T scale + bias + mask) v in the dtype of its inputs (fp64 here), plain torch."""
    Bw, N, C3 = qkv.shape
    d = C3 // 3 // h
    q, k, v = qkv.view(Bw, N, 3, h, d).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * scale + bias.unsqueeze(0)
    if mask is not None:
        nw = mask.shape[0]
        s = (s.view(Bw // nw, nw, h, N, N) + mask.to(s.dtype).view(1, nw, 1, N, N)).view(Bw, h, N, N)
    return (s.softmax(-1) @ v).transpose(1, 2).reshape(Bw, N, h * d)


@functools.lru_cache(maxsize=None)
def _swin_mask_cpu(img, ws, shift):
    from pytorch_distributedtraining_amd.models.swinir import SwinTransformerBlock
    blk = SwinTransformerBlock(12, (img, img), 2, window_size=ws, shift_size=shift)
    assert (blk.window_size, blk.shift_size) == (ws, shift)
    return blk._mask((img, img))


def _make_mask(kind, N, img, ws, shift):
    """None, Swin's own shift mask (the label path) or a random 0 / -100 mask with a zero diagonal (the dense path)."""
    from pytorch_distributedtraining_amd.ops import window_attention as WA
    if kind == "none":
        return None
    swin = _swin_mask_cpu(img, ws, shift).to(DEV)
    nw = swin.shape[0]
    assert nw == (img // ws) ** 2 and swin.shape[1:] == (N, N)
    if kind == "swin":
        assert WA.USE_LABELS and WA._mask_labels(swin) is not None, "the shift mask must take the label path"
        return swin
    g = torch.Generator(device=DEV).manual_seed(7)
    mask = torch.zeros(nw, N, N, device=DEV)
    mask[torch.rand(nw, N, N, device=DEV, generator=g) < 0.3] = -100.0
    mask[:, torch.arange(N), torch.arange(N)] = 0.0
    assert WA._mask_labels(mask) is None, "a random mask must take the dense path"
    return mask


class _HeadMajorGradConsumer(torch.autograd.Function):
    """Stands where ``ops.linear._LinearFn`` (in_hm) stands in the model: reads the attention output, and its backward
    hands the gradient back head-major, contiguous and tagged -- the tag set on a tensor created inside a backward."""

    @staticmethod
    def forward(ctx, o, N, h, d, o_is_hm):
        ctx.geom = (N, h, d)
        return _from_hm(o, N, h, d) if o_is_hm else o.clone()

    @staticmethod
    def backward(ctx, g):
        N, h, d = ctx.geom
        ghm = _to_hm(g, N, h, d)
        ghm._pdt_head_major = (N, d)
        return ghm, None, None, None, None


# (N, h, d, Bw, img, ws, shift): Bw a multiple of nw = (img / ws)^2.  Every shape satisfies _hm_ok and
# pdt_win_bwd_prep: d even, N C elem_bytes (C = h d) a multiple of 16 in bf16 and so in fp32, 3 N C 4 <= 96 KiB:
#   (64, 6, 10): 64 * 60 * 2 = 7,680 = 480 * 16      (16, 6, 10): 16 * 60 * 2 = 1,920 = 120 * 16
#   (49, 4, 16): 49 * 64 * 2 = 6,272 = 392 * 16      (36, 2, 14): 36 * 28 * 2 = 2,016 = 126 * 16
#   (64, 3, 2):  64 * 6 * 2 = 768 = 48 * 16          (64, 6, 16): 64 * 96 * 2 = 12,288 = 768 * 16 (fp32 qkv 73,728 B)
_SHAPES = [
    (64, 6, 10, 351, 24, 8, 4),   # SwinIR's; 88 groups of 4 windows > the backward's 85 workgroups per head, last partial
    (64, 6, 10, 9, 24, 8, 4),     # one partial group
    (16, 6, 10, 27, 12, 4, 2),    # window 4
    (49, 4, 16, 12, 14, 7, 3),    # N not a multiple of 16, d at the top of the MFMA range
    (36, 2, 14, 9, 18, 6, 3),
    (64, 3, 2, 18, 24, 8, 4),     # d at the bottom of the range
    (64, 6, 16, 9, 24, 8, 4),
]


def _draw(N, h, d, Bw, dt, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    C = h * d
    qkv = torch.randn(Bw, N, 3 * C, device=DEV, generator=g).to(dt)       # rounded first: both sides see these values
    bias = 0.5 * torch.randn(h, N, N, device=DEV, generator=g)
    do = torch.randn(Bw, N, C, device=DEV, generator=g).to(dt)
    return qkv, bias, do


@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("mask_kind", ["none", "swin", "dense"])
@pytest.mark.parametrize("N,h,d,Bw,img,ws,shift", _SHAPES)
def test_window_attention_layout_matrix(N, h, d, Bw, img, ws, shift, mask_kind, dt, spies):
    """{qkv untagged, given head-major} x {O token-major, head-major} x {dO untagged, tagged head-major} through
    ``_WindowAttnFn``: output, dqkv (always token-major) and dbias against fp64 autograd, and every variant against
    the all-token-major variant of the same case (same arithmetic, other addresses)."""
    from pytorch_distributedtraining_amd.ops import _lib
    from pytorch_distributedtraining_amd.ops import window_attention as WA
    assert N == ws * ws
    C, scale = h * d, d ** -0.5
    if Bw == 351:       # more groups of 4 windows than one pass of the backward grid covers, and a partial last group
        assert math.ceil(Bw / 4) > _lib.require().pdt_win_attn_mfma_grid(Bw, h) and Bw % 4
    qkv, bias, do = _draw(N, h, d, Bw, dt, seed=N * 1000 + Bw)
    mask = _make_mask(mask_kind, N, img, ws, shift)
    qr, br = qkv.double().requires_grad_(), bias.double().requires_grad_()
    o_ref = _ref64(qr, br, None if mask is None else mask.double(), h, scale)
    o_ref.backward(do.double())
    tol = 2e-2 if dt == BF16 else 1e-4

    def run(given, out_hm, g_tagged):
        spies.clear()
        if given:
            q_in = _to_hm(qkv, N, 3 * h, d).detach().requires_grad_()
            q_in._pdt_head_major = (N, d)
        else:
            q_in = qkv.clone().requires_grad_()
        b_in = bias.clone().requires_grad_()
        o = WA._WindowAttnFn.apply(q_in, b_in, mask, h, scale, out_hm)
        ctx = o.grad_fn
        assert ctx.mfma == ("bf16" if dt == BF16 else "f32") and ctx.hm is True
        tag = _tag(o)
        assert (tag == (N, d)) == (dt == BF16 and out_hm and ctx.hm) and tag in (None, (N, d))
        assert ctx.o_hm == (tag is not None)
        assert spies.qkv == [(N, d) if given else None]
        if g_tagged:
            o_tm = _HeadMajorGradConsumer.apply(o, N, h, d, tag is not None)
            o_tm.backward(do)
            o_tm = o_tm.detach()
        else:
            o.backward(do)          # an untagged dO is token-major, whichever layout O has
            o_tm = _from_hm(o.detach(), N, h, d) if tag is not None else o.detach()
        assert spies.do == [(N, d) if g_tagged else None] and spies.o_hm == [tag is not None]
        assert q_in.grad.shape == qkv.shape and _tag(q_in.grad) is None
        return {"o": o_tm, "dqkv": q_in.grad, "dbias": b_in.grad}

    outs = [False, True]        # fp32: a requested head-major output stays token-major and untagged (asserted in run)
    base = None
    for given in (False, True):
        for out_hm in outs:
            for g_tagged in (False, True):
                label = f"[qkv {'given' if given else 'plain'}, O {'hm' if out_hm else 'tm'}, " \
                        f"dO {'tagged' if g_tagged else 'plain'}]"
                r = run(given, out_hm, g_tagged)
                _report(label, [("o", rel_err(r["o"], o_ref), tol), ("dqkv", rel_err(r["dqkv"], qr.grad), 2 * tol),
                                ("dbias", rel_err(r["dbias"], br.grad), 2 * tol)])
                if base is None:
                    base = r
                else:
                    _same(label, r, base)


@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "fp32"])
def test_window_attention_bias_grad_is_reproducible(dt):
    """The bias gradient's sum over a workgroup's four waves runs in a fixed order: the same backward twice gives the
    same bits (a bf16 table gradient rounded from it would otherwise differ by an ulp between two runs, and the
    layout comparisons above and in part B could not hold their bounds)."""
    from pytorch_distributedtraining_amd.ops import window_attention as WA
    N, h, d, Bw = 64, 6, 10, 351
    qkv, bias, do = _draw(N, h, d, Bw, dt, seed=23)
    grads = []
    for _ in range(3):
        b_in = bias.clone().requires_grad_()
        WA._WindowAttnFn.apply(qkv.clone().requires_grad_(), b_in, None, h, d ** -0.5).backward(do)
        grads.append(b_in.grad)
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0], grads[2])


@pytest.mark.parametrize("mask_kind", ["none", "swin"])
def test_window_attention_table_head_major(mask_kind, spies):
    """``_WindowAttnTableFn`` with qkv given head-major, O head-major and dO tagged, at SwinIR's shape (351 windows):
    the relative-position TABLE gradient against fp64 ``table[index]`` autograd."""
    from pytorch_distributedtraining_amd.models.swinir import WindowAttention
    from pytorch_distributedtraining_amd.ops import window_attention as WA
    N, h, d, Bw = 64, 6, 10, 351
    scale = d ** -0.5
    qkv, _, do = _draw(N, h, d, Bw, BF16, seed=11)
    index = WindowAttention(h * d, 8, h).relative_position_index.to(DEV)
    table = (0.5 * torch.randn(225, h, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))).to(BF16)
    mask = _make_mask(mask_kind, N, 24, 8, 4)
    qr, tr = qkv.double().requires_grad_(), table.double().requires_grad_()
    rel = tr[index.reshape(-1)].view(N, N, h).permute(2, 0, 1)
    o_ref = _ref64(qr, rel, None if mask is None else mask.double(), h, scale)
    o_ref.backward(do.double())

    def run(fast):
        spies.clear()
        q_in = (_to_hm(qkv, N, 3 * h, d).detach() if fast else qkv.clone()).requires_grad_()
        if fast:
            q_in._pdt_head_major = (N, d)
        t_in = table.clone().requires_grad_()
        o = WA._WindowAttnTableFn.apply(q_in, t_in, index, mask, h, scale, fast)
        assert _tag(o) == ((N, d) if fast else None) and o.grad_fn.o_hm == fast and o.grad_fn.hm is True
        if fast:
            o_tm = _HeadMajorGradConsumer.apply(o, N, h, d, True)
            o_tm.backward(do)
        else:
            o_tm = o
            o.backward(do)
        assert spies.qkv == [(N, d) if fast else None] and spies.do == [(N, d) if fast else None]
        assert t_in.grad.dtype == BF16 and _tag(q_in.grad) is None
        return {"o": o_tm.detach(), "dqkv": q_in.grad, "dtable": t_in.grad}

    base, fast = run(False), run(True)
    for label, r in (("[token-major]", base), ("[given, O hm, dO tagged]", fast)):
        _report(label, [("o", rel_err(r["o"], o_ref), 2e-2), ("dqkv", rel_err(r["dqkv"], qr.grad), 4e-2),
                        ("dtable", rel_err(r["dtable"], tr.grad), 4e-2)])
    _same("[given, O hm, dO tagged]", fast, base)


@pytest.mark.parametrize("why", ["hook", "small"])
def test_linear_from_head_major_last_resort_returns_tagged_grad(why, spies):
    """A head-major attention output handed to a projection that cannot read it (a hook on it / fewer rows than the
    narrow GEMM takes): ``linear_from_head_major`` runs ``module(token-major copy)``, and the gradient it returns to the attention is
    head-major AND tagged -- an untagged one would be read as token-major (wrong dqkv / dbias, no error)."""
    import pytorch_distributedtraining_amd.ops.linear as L
    from pytorch_distributedtraining_amd.ops import window_attention as WA
    N, h, d, Bw = 64, 6, 10, 9
    C, scale = h * d, d ** -0.5
    qkv, bias, dy = _draw(N, h, d, Bw, BF16, seed=5)
    mask = _make_mask("swin", N, 24, 8, 4)
    torch.manual_seed(0)
    proj = L.Linear(C, C).to(DEV).to(BF16)
    seen = []
    if why == "hook":
        proj.register_forward_hook(lambda m, i, o: seen.append(i[0].detach().clone()))
    q_in = _to_hm(qkv, N, 3 * h, d).detach().requires_grad_()
    q_in._pdt_head_major = (N, d)
    b_in = bias.clone().requires_grad_()
    o = WA._WindowAttnFn.apply(q_in, b_in, mask, h, scale, True)
    assert _tag(o) == (N, d)
    y = L.linear_from_head_major(proj, o)
    y.backward(dy)
    qr, br = qkv.double().requires_grad_(), bias.double().requires_grad_()
    wr, pbr = proj.weight.detach().double().requires_grad_(), proj.bias.detach().double().requires_grad_()
    o_ref = _ref64(qr, br, mask.double(), h, scale)
    y_ref = F.linear(o_ref, wr, pbr)
    y_ref.backward(dy.double())
    if why == "hook":
        assert len(seen) == 1
        _report(why, [("hook input (token-major O)", rel_err(seen[0], o_ref), 2e-2)])
    _report(why, [("y", rel_err(y, y_ref), 2e-2), ("dqkv", rel_err(q_in.grad, qr.grad), 4e-2),
                  ("dbias", rel_err(b_in.grad, br.grad), 4e-2), ("dW", rel_err(proj.weight.grad, wr.grad), 4e-2),
                  ("db", rel_err(proj.bias.grad, pbr.grad), 4e-2)])
    assert spies.do == [(N, d)] and spies.o_hm == [True]


# ------------------------------------------------------------------------------------------------
# B. dispatch and fallbacks on a real block
# ------------------------------------------------------------------------------------------------
_GRADS = ["attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias",
          "attn.relative_position_bias_table", "norm1.weight", "mlp.fc1.weight", "mlp.fc2.weight"]


def _run_block(blk, x, res, x_grad=True, fwd_ctx=contextlib.nullcontext):
    blk.zero_grad(set_to_none=True)
    xi = x.clone().requires_grad_(x_grad)
    with fwd_ctx():
        y = blk(xi, res)
    wide = y.double() if y.dtype == torch.float64 else y.float()
    (wide.square().sum() / 1024).backward()
    out = {"y": y.detach(), "dx": xi.grad}
    params = dict(blk.named_parameters())
    for n in _GRADS:
        out[n] = params[n].grad.detach().clone()
    return out


@functools.lru_cache(maxsize=None)
def _block_case(res, batch, ws, shift, dt):
    """(CPU master block in ``dt``, CPU input, fp64 CPU results incl. the projection's input) -- built once per
    geometry and shared, never modified: each test runs a deep copy of the master on the GPU."""
    from pytorch_distributedtraining_amd.models.swinir import SwinTransformerBlock
    torch.manual_seed(0)
    master = SwinTransformerBlock(60, (res, res), 6, window_size=ws, shift_size=shift)
    with torch.no_grad():        # biases, norms and the table away from their (near-)zero initial values
        master.attn.relative_position_bias_table.normal_(0, 0.5)
        for n in (master.norm1, master.norm2):
            n.weight.add_(0.1 * torch.randn_like(n.weight))
            n.bias.add_(0.1 * torch.randn_like(n.bias))
    master = master.to(dt)
    x = torch.randn(batch, res * res, 60).to(dt)
    oracle = copy.deepcopy(master).double()
    proj_in = []
    hd = oracle.attn.proj.register_forward_pre_hook(lambda m, a: proj_in.append(a[0].detach().clone()))
    ref = _run_block(oracle, x.double(), (res, res))
    hd.remove()
    assert len(proj_in) == 1
    ref["proj_in"] = proj_in[0]
    return master, x, ref


def _vs_oracle(label, got, ref, x_grad=True):
    rows = []
    for k in ["y", "dx"] + _GRADS:
        if k == "dx" and not x_grad:
            assert got["dx"] is None
            continue
        rows.append((k, rel_err(got[k], ref[k]), 2e-2 if k == "y" else 4e-2))
    _report(label, rows)


def _twin(blk, x, res, spies, monkeypatch, **kw):
    """The same block on the token-major path of the same kernels."""
    import pytorch_distributedtraining_amd.models.swinir as S
    import pytorch_distributedtraining_amd.ops.linear as L
    with monkeypatch.context() as m:
        m.setattr(L, "HEAD_MAJOR_QKV", False)
        m.setattr(S, "HEAD_MAJOR_PROJ", False)
        spies.clear()
        r = _run_block(blk, x, res, **kw)
        assert spies.qkv == [None] and spies.proj_in == [None] and spies.do == [None] and spies.o_hm == [False]
    return r


_BASE = (32, 16, 8, 4, BF16)     # 16 x 32 x 32 = 16,384 tokens, N = 64, Bw = 256


def _gpu_block(case):
    master, x, ref = _block_case(*case)
    return copy.deepcopy(master).to(DEV), x.to(DEV), ref, (case[0], case[0])


def test_block_all_fast_paths(spies, monkeypatch):
    """Case 1: qkv given head-major, O head-major, dO tagged."""
    blk, x, ref, res = _gpu_block(_BASE)
    got = _run_block(blk, x, res)
    assert spies.qkv == [(64, 10)] and spies.proj_in == [(64, 10)] and spies.do == [(64, 10)]
    assert spies.o_hm == [True] and spies.hm == [True]
    _vs_oracle("fast", got, ref)
    _same("fast", got, _twin(blk, x, res, spies, monkeypatch))


def test_block_forward_hook_on_proj(spies, monkeypatch):
    """Case 2: a forward hook on attn.proj sees the module's usual call once, on the token-major attention output;
    the attention is then not asked for a head-major output (or, if it were, its dO would have to come back tagged)."""
    blk, x, ref, res = _gpu_block(_BASE)
    seen = []
    blk.attn.proj.register_forward_hook(lambda m, i, o: seen.append(i[0].detach().clone()))
    got = _run_block(blk, x, res)
    o_hm, do = list(spies.o_hm), list(spies.do)
    assert len(seen) == 1
    _report("proj hook", [("hook input", rel_err(seen[0], ref["proj_in"]), 2e-2)])
    _vs_oracle("proj hook", got, ref)          # (numbers first: they are the finding when a path is wrong)
    assert spies.qkv == [(64, 10)]
    assert o_hm == [False] or do == [(64, 10)], (o_hm, do)
    assert o_hm == [False] and spies.proj_in == [None] and do == [None]
    seen.clear()
    _same("proj hook", got, _twin(blk, x, res, spies, monkeypatch))
    assert len(seen) == 1


def test_block_pre_hook_on_qkv(spies, monkeypatch):
    """Case 3: a forward pre-hook on attn.qkv -- the qkv reaching the attention is token-major and untagged, the
    attention output still goes head-major."""
    blk, x, ref, res = _gpu_block(_BASE)
    fired = []
    blk.attn.qkv.register_forward_pre_hook(lambda m, a: fired.append(1))
    got = _run_block(blk, x, res)
    assert len(fired) == 1
    assert spies.qkv == [None] and spies.proj_in == [(64, 10)] and spies.do == [(64, 10)] and spies.o_hm == [True]
    _vs_oracle("qkv pre-hook", got, ref)
    _same("qkv pre-hook", got, _twin(blk, x, res, spies, monkeypatch))


def test_block_global_forward_hook(spies):
    """Case 4: a global module forward hook puts every projection on its usual module call."""
    blk, x, ref, res = _gpu_block(_BASE)
    fired = []
    handle = torch.nn.modules.module.register_module_forward_hook(lambda m, i, o: fired.append(type(m).__name__))
    try:
        got = _run_block(blk, x, res)
    finally:
        handle.remove()
    assert fired.count("Linear") >= 2 and fired.count("SwinTransformerBlock") == 1
    _vs_oracle("global hook", got, ref)
    assert spies.qkv == [None]
    assert spies.o_hm == [False] or spies.do == [(64, 10)], (spies.o_hm, spies.do)
    assert spies.o_hm == [False] and spies.proj_in == [None] and spies.do == [None]


def test_block_inside_fp8_autocast(spies):
    """Case 5: inside ``fp8_autocast()`` (60-wide Linears never take the fp8 GEMM, but ``fp8_enabled()`` holds)."""
    from pytorch_distributedtraining_amd.ops.fp8 import fp8_autocast
    blk, x, ref, res = _gpu_block(_BASE)
    got = _run_block(blk, x, res, fwd_ctx=fp8_autocast)
    _vs_oracle("fp8 region", got, ref)
    assert spies.qkv == [None]
    assert spies.o_hm == [False] or spies.do == [(64, 10)], (spies.o_hm, spies.do)
    assert spies.o_hm == [False] and spies.proj_in == [None] and spies.do == [None]


def test_block_narrow_off(spies, monkeypatch):
    """Case 6: PDT_NARROW=0 -- qkv from the library GEMM (token-major, untagged); the projection still reads the
    head-major output (its head-major route does not consult the timing pick).  (No token-major twin at 1e-5: its
    projection runs the library GEMM, other arithmetic.)"""
    import pytorch_distributedtraining_amd.ops.linear as L
    monkeypatch.setattr(L, "NARROW", "0")
    blk, x, ref, res = _gpu_block(_BASE)
    got = _run_block(blk, x, res)
    assert spies.qkv == [None] and spies.proj_in == [(64, 10)] and spies.do == [(64, 10)] and spies.o_hm == [True]
    _vs_oracle("narrow off", got, ref)


def test_block_bf16_autocast_over_fp32(spies):
    """Case 7: bf16 autocast over fp32 parameters and an fp32 input."""
    case = (32, 16, 8, 4, F32)
    blk, x, ref, res = _gpu_block(case)
    got = _run_block(blk, x, res, fwd_ctx=lambda: torch.autocast("cuda", torch.bfloat16))
    assert all(got[k].dtype == F32 for k in _GRADS)
    assert spies.qkv == [(64, 10)] and spies.proj_in == [(64, 10)] and spies.do == [(64, 10)] and spies.o_hm == [True]
    _vs_oracle("autocast", got, ref)


def test_block_window_4(spies, monkeypatch):
    """Case 8: window 4, shift 2 on 128 x 128 (N = 16, Bw = 1024): 16-token tags; the projection's weight gradient
    is NOT the 64-token head-major narrow kernel but ``wgrad`` on a token-major copy.  (No twin at 1e-5: the twin's
    weight gradient may run another GEMM.)"""
    import pytorch_distributedtraining_amd.ops.linear as L
    blk, x, ref, res = _gpu_block((128, 1, 4, 2, BF16))
    real_nw, real_tm, real_wg = L.narrow_wgrad, L._token_major, L.wgrad
    hm_wgrads, copies, on_copy = [], [], []

    def nw(dy2, x2, out_dtype, x_hm_d=0):
        hm_wgrads.append(x_hm_d)
        return real_nw(dy2, x2, out_dtype, x_hm_d=x_hm_d)

    def tm(*a):
        copies.append(real_tm(*a))
        return copies[-1]

    def wg(dy2, x2, *a, **k):
        on_copy.append(any(x2 is c for c in copies))
        return real_wg(dy2, x2, *a, **k)
    monkeypatch.setattr(L, "narrow_wgrad", nw)
    monkeypatch.setattr(L, "_token_major", tm)
    monkeypatch.setattr(L, "wgrad", wg)
    got = _run_block(blk, x, res)
    assert spies.qkv == [(16, 10)] and spies.proj_in == [(16, 10)] and spies.do == [(16, 10)] and spies.o_hm == [True]
    assert not any(hm_wgrads), hm_wgrads
    assert any(on_copy), "the head-major backward must take wgrad(dy, token-major copy of O)"
    _vs_oracle("window 4", got, ref)


def test_block_proj_dgrad_off_narrow(spies, monkeypatch):
    """Case 9: the projection's data gradient off the narrow kernel (``narrow_ok`` refuses inside
    ``_backward_head_major`` only): the attention gets a token-major, untagged dO with a head-major O."""
    import pytorch_distributedtraining_amd.ops.linear as L
    blk, x, ref, res = _gpu_block(_BASE)
    inside, refused = [0], []
    real_bhm, real_ok = L._LinearFn._backward_head_major, L.narrow_ok

    def bhm(*a):
        inside[0] += 1
        try:
            return real_bhm(*a)
        finally:
            inside[0] -= 1

    def ok(*a, **k):
        if inside[0]:
            refused.append(1)
            return False
        return real_ok(*a, **k)
    monkeypatch.setattr(L._LinearFn, "_backward_head_major", staticmethod(bhm))
    monkeypatch.setattr(L, "narrow_ok", ok)
    got = _run_block(blk, x, res)
    assert refused == [1]
    assert spies.qkv == [(64, 10)] and spies.proj_in == [(64, 10)] and spies.do == [None] and spies.o_hm == [True]
    _vs_oracle("proj dgrad on mm", got, ref)


def test_block_input_without_grad(spies, monkeypatch):
    """Case 10: an input that needs no gradient -- the parameter gradients are unchanged."""
    blk, x, ref, res = _gpu_block(_BASE)
    got = _run_block(blk, x, res, x_grad=False)
    assert spies.qkv == [(64, 10)] and spies.proj_in == [(64, 10)] and spies.do == [(64, 10)] and spies.o_hm == [True]
    _vs_oracle("no input grad", got, ref, x_grad=False)
    _same("no input grad", got, _twin(blk, x, res, spies, monkeypatch, x_grad=False))


def test_mlp_forward_hook_on_fc2(monkeypatch):
    """A forward hook on mlp.fc2 (fp32: the unfused MLP whose residual rides in fc2's GEMM) fires once -- the module's
    usual call -- and output and gradients are those of the unhooked run."""
    import pytorch_distributedtraining_amd.models.swinir as S
    import pytorch_distributedtraining_amd.ops.linear as L
    monkeypatch.setattr(L, "NARROW", "1")
    master, x, _ = _block_case(32, 16, 8, 4, F32)
    blk, x = copy.deepcopy(master).to(DEV), x.to(DEV)
    fused_calls = []
    real_lr = S.linear_residual

    def lr(*a):
        fused_calls.append(1)
        return real_lr(*a)
    monkeypatch.setattr(S, "linear_residual", lr)
    plain = _run_block(blk, x, (32, 32))
    assert fused_calls == [1], "the unhooked fp32 MLP adds its residual in fc2's GEMM"
    fired = []
    blk.mlp.fc2.register_forward_hook(lambda m, i, o: fired.append(o.shape[-1]))
    hooked = _run_block(blk, x, (32, 32))
    assert fired == [60] and fused_calls == [1]
    _same("fc2 hook", hooked, plain)


# ------------------------------------------------------------------------------------------------
# D. fused L1 in the same training path
# ------------------------------------------------------------------------------------------------
def test_l1_bf16_output_against_fp32_target():
    """models.losses._l1 with a bf16 output and an fp32 target that differs from it by a quarter of the output's
    bf16 spacing: the difference is taken in fp32 (F.l1_loss's promotion), not after rounding the target to bf16."""
    from pytorch_distributedtraining_amd.models.losses import _l1
    g = torch.Generator(device=DEV).manual_seed(0)
    shape = (2, 3, 32, 48)
    a = (1.0625 + 0.8 * torch.rand(shape, device=DEV, generator=g)).to(BF16)
    _, e = torch.frexp(a.float())                        # a = m 2^e, m in [0.5, 1): bf16 spacing 2^(e - 8)
    sign = torch.where(torch.rand(shape, device=DEV, generator=g) < 0.5, -1.0, 1.0)
    b = a.float() + sign * 0.25 * torch.ldexp(torch.ones_like(sign), e - 8)
    assert torch.equal(b.to(BF16), a) and not torch.equal(b, a.float())
    a.requires_grad_()
    loss = _l1(a, b)
    loss.backward()
    ad = a.detach().double().requires_grad_()
    ref = F.l1_loss(ad, b.double())
    ref.backward()
    assert torch.equal(torch.sign(ad.grad), -sign.double())
    print(f"loss {loss.item():.9e}, fp64 {ref.item():.9e}")
    assert abs(loss.item() - ref.item()) <= 1e-5 * ref.item()
    assert a.grad.dtype == BF16 and torch.equal(torch.sign(a.grad.double()), torch.sign(ad.grad))
    worst = ((a.grad.double() - ad.grad).abs() / ad.grad.abs()).max().item()
    print(f"gradient: worst relative error {worst:.3e}")
    assert worst <= 2.0 ** -8


@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "fp32"])
def test_l1_backward_twice_with_upstream_scale(dt):
    """ops.l1 backward must not scale its saved buffer in place: two backward passes of a retained graph with an
    upstream gradient of 3 both give 3 sign(a - b) / n (n a power of two: exact in both dtypes)."""
    from pytorch_distributedtraining_amd.ops import l1 as L1
    g = torch.Generator(device=DEV).manual_seed(1)
    shape = (4, 8, 16, 32)
    a = torch.randn(shape, device=DEV, generator=g).to(dt).requires_grad_()
    side = torch.where(torch.rand(shape, device=DEV, generator=g) < 0.5, -1.0, 1.0)
    b = (a.detach().float() + side * (0.5 + torch.rand(shape, device=DEV, generator=g))).to(dt)     # never a: no sign(0)
    assert L1.FUSED and not (a.detach() == b).any()
    loss = 3 * L1.l1_loss(a, b)
    assert type(loss.grad_fn.next_functions[0][0]).__name__.startswith("_L1Fn")
    loss.backward(retain_graph=True)
    g1 = a.grad.clone()
    a.grad = None
    loss.backward(retain_graph=True)
    g2 = a.grad.clone()
    want = (3 * torch.sign(a.detach().double() - b.double()) / a.numel())
    assert torch.equal(g1.double(), want)
    assert torch.equal(g2, g1)
