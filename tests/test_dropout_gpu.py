"""Mask-free dropout on the MI355X: the standalone kernels, the fused dropout + residual add + norm site, the
composite path outside the fused kernel's contract and GPT-2 with dropout, all against torch references built
with the numpy mask of tests/dropout_ref.py (the mask is known exactly, so dropout adds one multiply to the
error budget of the existing add + norm tests and their tolerances carry over)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dropout_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
P = 0.1
KEY = -0x0123456789ABCDEF          # high word set, negative as int64


def rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


@pytest.fixture(autouse=True)
def _seed():
    torch.manual_seed(0)


def _key(v=KEY):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


@functools.lru_cache(maxsize=None)
def _ref_keep_np(numel, key, p):
    m = R.keep_mask(numel, key, p)
    m.setflags(write=False)
    return m


def ref_keep(shape, key=KEY, p=P):
    """The reference mask of a contiguous tensor of ``shape`` on the GPU (computed once per (numel, key, p))."""
    numel = int(np.prod(shape))
    return torch.from_numpy(_ref_keep_np(numel, key, p).copy()).view(*shape).to(DEV)


# ---- standalone kernels -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [KEY, 0x7123456789ABCDEF, 5])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_dropout_kernels_match_reference_mask(dt, key):
    from pytorch_distributedtraining_amd.ops import dropout as D
    numel = 8 * 1000 + 3
    x = torch.ones(numel, device=DEV, dtype=dt, requires_grad=True)
    y = D.dropout(x, P, _key(key))
    y.backward(torch.ones_like(y))
    keep = ref_keep((numel,), key)
    scale = torch.tensor(float(R.quantise(P)[1]), device=DEV).to(dt)       # scale rounded to the dtype
    want = torch.where(keep, scale, torch.zeros((), device=DEV, dtype=dt))
    assert torch.equal(y != 0, keep) and torch.equal(y.detach(), want)
    assert torch.equal(x.grad != 0, keep) and torch.equal(x.grad, want)
    assert 0 < int(keep.sum()) < numel


def test_dropout_module_gpu():
    from pytorch_distributedtraining_amd.ops import Dropout
    m = Dropout(0.5).to(DEV)
    x = torch.randn(33, 77, device=DEV, dtype=torch.bfloat16)
    torch.manual_seed(1)
    a = m(x)
    torch.manual_seed(1)
    assert torch.equal(a, m(x)) and not torch.equal(a, m(x))
    kept = a != 0
    assert torch.equal(a[kept], (x.float() * 2).bfloat16()[kept]) and 0.4 < kept.float().mean().item() < 0.6
    assert m.eval()(x) is x


@pytest.mark.parametrize("cdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("rows,N", [(37, 96), (300, 768), (67, 2048), (45, 4104), (50, 60)])
def test_dropout_bwd_column_sums(rows, N, dt, cdt):
    """dx from the regenerated mask plus, in the same pass, the column sums of dx as stored.  Narrow (N < 2048)
    and wide kernels, several row chunks, a last column group that ends inside its 2048 columns; N = 60 sums
    through the package's column-sum kernel.  Bound: fp32 summation of n terms in any order errs by at most
    n * 2^-24 * sum|dx| per column (fp32 output), plus one rounding (2^-8 relative) for a bf16 output."""
    from pytorch_distributedtraining_amd.ops import dropout as D
    thr, scale = D.quantise(P)
    dy = torch.randn(rows, N, device=DEV, dtype=dt)
    dx, cs = D.dropout_bwd(dy, _key(), thr, scale, cdt)
    keep = ref_keep((rows, N))
    want = torch.where(keep, (dy.float() * np.float32(scale)).to(dt), torch.zeros((), device=DEV, dtype=dt))
    assert torch.equal(dx, want)
    assert cs.dtype == cdt and cs.shape == (N,)
    exact = dx.double().sum(0)
    bound = rows * 2.0 ** -24 * dx.double().abs().sum(0)
    if cdt == torch.bfloat16:
        bound = bound + 2.0 ** -8 * exact.abs()
    assert bool(((cs.double() - exact).abs() <= bound + 1e-30).all()), ((cs.double() - exact).abs() / (bound + 1e-30)).max()


# ---- the fused site and the composite path ----------------------------------------------------------------------
def _site_case(rms, N, mode, rbias, rows, xdt=torch.bfloat16, wdt=torch.bfloat16, fused=True):
    from pytorch_distributedtraining_amd.ops import norms
    x = torch.randn(rows, N, device=DEV, dtype=xdt, requires_grad=True)
    r = torch.randn(rows, N, device=DEV, dtype=xdt, requires_grad=True)
    w = (1 + 0.1 * torch.randn(N, device=DEV)).to(wdt).requires_grad_()
    b = None if rms else (0.1 * torch.randn(N, device=DEV)).to(wdt).requires_grad_()
    rb = (0.5 * torch.randn(N, device=DEV)).to(wdt).requires_grad_() if rbias else None
    assert norms.drop_add_norm_ok(x, r, w, rb) == fused
    y, s = norms.add_norm(x, r, w, b, 1e-5, rms=rms, r_bias=rb, dropout=(P, _key(), mode))
    dy, ds = torch.randn_like(y), torch.randn_like(s)
    torch.autograd.backward([y, s], [dy, ds])

    keep = ref_keep((rows, N))
    scale = float(R.quantise(P)[1])
    xr, rr, wr = (t.detach().float().requires_grad_() for t in (x, r, w))
    br = None if rms else b.detach().float().requires_grad_()
    rbr = rb.detach().float().requires_grad_() if rbias else None
    zero = torch.zeros((), device=DEV)
    if mode == "residual":
        sr = xr + torch.where(keep, (rr if rb is None else rr + rbr) * scale, zero)
    else:
        sr = torch.where(keep, (xr + rr) * scale, zero)
    yr = sr * torch.rsqrt(sr.pow(2).mean(-1, keepdim=True) + 1e-5) * wr if rms else F.layer_norm(sr, (N,), wr, br, 1e-5)
    torch.autograd.backward([yr, sr], [dy.float(), ds.float()])

    errs = dict(s=rel_err(s, sr), y=rel_err(y, yr), dx=rel_err(x.grad, xr.grad), dr=rel_err(r.grad, rr.grad),
                dw=rel_err(w.grad, wr.grad))
    print(dict(rms=rms, N=N, mode=mode, rbias=rbias, rows=rows), errs)
    assert errs["s"] < 1e-2 and errs["y"] < 1e-2, errs
    assert errs["dx"] < 2e-2 and errs["dr"] < 2e-2 and errs["dw"] < 2e-2, errs
    if not rms:
        assert rel_err(b.grad, br.grad) < 2e-2
    if rbias:
        assert rel_err(rb.grad, rbr.grad) < 2e-2
        # the column sum of the stored dr (fp32 accumulation of the rounded values)
        assert rel_err(rb.grad, r.grad.float().sum(0)) < 1e-2
    # the mask itself, exactly: the kept / dropped pattern of r's gradient and of the stored sum
    assert torch.equal(r.grad != 0, keep)
    if mode == "residual":
        assert torch.equal(s.detach()[~keep], x.detach()[~keep])          # a dropped element's s is bitwise x
    else:
        assert torch.equal(s.detach()[~keep], torch.zeros_like(s.detach()[~keep]))
        assert torch.equal(x.grad, r.grad)


SITES = [("residual", False), ("residual", True), ("sum", False)]


@pytest.mark.parametrize("mode,rbias", SITES)
@pytest.mark.parametrize("rms", [False, True])
@pytest.mark.parametrize("N", [96, 128, 768, 1280, 2048])
def test_fused_dropout_add_norm(rms, N, mode, rbias):
    """N = 96 and 1280 end inside a 512-column slab; 128 / 768 / 2048 take 1 / 2 / 4 slabs."""
    _site_case(rms, N, mode, rbias, rows=37)


@pytest.mark.parametrize("mode,rbias", SITES)
@pytest.mark.parametrize("rms", [False, True])
def test_fused_dropout_add_norm_grid_stride(rms, mode, rbias):
    """3000 x 2048 as in test_fused_add_norm (rows past one block per wave, 64-bit element indices per row)."""
    _site_case(rms, 2048, mode, rbias, rows=3000)


@pytest.mark.parametrize("xdt,wdt", [(torch.float32, torch.float32), (torch.bfloat16, torch.float32),
                                     (torch.float32, torch.bfloat16)])
@pytest.mark.parametrize("mode,rbias", SITES)
def test_fused_dropout_add_norm_dtypes(xdt, wdt, mode, rbias):
    _site_case(False, 768, mode, rbias, rows=37, xdt=xdt, wdt=wdt)


@pytest.mark.parametrize("mode,rbias", SITES)
@pytest.mark.parametrize("rms", [False, True])
@pytest.mark.parametrize("N", [60, 4096])
def test_dropout_add_norm_composite(rms, N, mode, rbias):
    """Outside the fused kernel's contract (N % 8 != 0, N > 2048): dropout() composed with add_norm, same results."""
    _site_case(rms, N, mode, rbias, rows=37, fused=False)


def test_add_norm_dropout_off_is_todays_path():
    from pytorch_distributedtraining_amd.ops.norms import add_norm
    x = torch.randn(37, 768, device=DEV, dtype=torch.bfloat16)
    r = torch.randn(37, 768, device=DEV, dtype=torch.bfloat16)
    w = torch.ones(768, device=DEV, dtype=torch.bfloat16)
    b = torch.zeros(768, device=DEV, dtype=torch.bfloat16)
    y0, s0 = add_norm(x, r, w, b)
    for d in (None, (0.0, _key(), "residual")):
        y1, s1 = add_norm(x, r, w, b, dropout=d)
        assert torch.equal(y0, y1) and torch.equal(s0, s1)


# ---- GPT-2 -------------------------------------------------------------------------------------------------------
def _fixed_keys(n, device):
    return (torch.arange(n, dtype=torch.int64) * 0x0F1E2D3C4B5A6978 - 0x1234567).to(device)


@pytest.mark.parametrize("ckpt", [False, True])
def test_gpt2_dropout_every_grad_matches_fp32_reference(ckpt, monkeypatch):
    """The set-up of test_gpt2_every_grad_matches_fp32_reference with embd_pdrop = resid_pdrop = 0.1 and the keys
    fixed on both sides: the bf16 model on the HIP kernels against the fp32 CPU model (torch-op masks).  A wrong
    mask at any site is an O(1) error in every gradient upstream of it."""
    from pytorch_distributedtraining_amd.models import build_gpt2
    from pytorch_distributedtraining_amd.ops import attention as A
    from pytorch_distributedtraining_amd.ops import dropout as D
    from pytorch_distributedtraining_amd.ops import norms as NM
    monkeypatch.setattr(D, "draw_keys", _fixed_keys)
    kw = dict(n_embd=256, n_head=2, n_layer=3, embd_pdrop=0.1, resid_pdrop=0.1)
    torch.manual_seed(0)
    ref = build_gpt2("gpt2-tiny", **kw)
    x = torch.randint(0, 512, (4, 129))
    ref(x[:, :-1], labels=x[:, 1:]).backward()
    m = build_gpt2("gpt2-tiny", activation_checkpointing=ckpt, **kw)
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).bfloat16()
    xd = x.to(DEV)
    seen = []
    orig = NM._drop_add_norm

    def site(x_, r_, weight, bias, eps, rms, r_bias, r_colsum, p, key, mode):
        assert NM.drop_add_norm_ok(x_, r_, weight, r_bias)                  # the fused kernel runs at every site
        seen.append((int(key.item()), mode))
        return orig(x_, r_, weight, bias, eps, rms, r_bias, r_colsum, p, key, mode)

    monkeypatch.setattr(NM, "_drop_add_norm", site)
    m(xd[:, :-1], labels=xd[:, 1:]).backward()
    L = 3
    keys = [int(k) for k in _fixed_keys(2 * L + 1, "cpu")]
    fwd = [(keys[0], "sum")] + [(k, "residual") for k in keys[1:]]
    assert seen[:2 * L + 1] == fwd
    if ckpt:    # the recompute (last block first) sees the keys of its forward
        assert seen[2 * L + 1:] == [fwd[2 * i + j] for i in reversed(range(L)) for j in (0, 1)]
    else:
        assert len(seen) == 2 * L + 1
    assert not [e for e in A._BIAS_GRADS.values() if e[0]() is not None]      # every stashed colsum consumed
    grads = dict(ref.named_parameters())
    worst = {}
    for n, p in m.named_parameters():
        g, want = p.grad.float().cpu(), grads[n].grad
        worst[n] = rel_err(g, want)
    print({n: round(e, 4) for n, e in worst.items() if "c_proj.bias" in n}, max(worst.values()))
    for n, e in worst.items():
        assert e < 4e-2, (n, e)
    assert sum("c_proj.bias" in n for n in worst) == 2 * L


def test_gpt2_dropout_eval_is_todays_model():
    from pytorch_distributedtraining_amd.models import build_gpt2
    torch.manual_seed(0)
    base = build_gpt2("gpt2-tiny", n_embd=256, n_head=2, n_layer=3)
    m = build_gpt2("gpt2-tiny", n_embd=256, n_head=2, n_layer=3, embd_pdrop=0.1, resid_pdrop=0.1)
    m.load_state_dict(base.state_dict())
    base, m = base.to(DEV).bfloat16().eval(), m.to(DEV).bfloat16().eval()
    x = torch.randint(0, 512, (4, 128), device=DEV)
    with torch.no_grad():
        assert torch.equal(m(x), base(x))


def test_gpt2_dropout_graph_replays_draw_fresh_keys():
    """The keys live in device memory and come from torch's capture-aware generator: every replay of a captured
    training-mode forward drops a different set of elements; eager runs follow manual_seed."""
    from pytorch_distributedtraining_amd.models import build_gpt2
    torch.manual_seed(0)
    m = build_gpt2("gpt2-tiny", n_embd=256, n_head=2, n_layer=2, embd_pdrop=0.1, resid_pdrop=0.1)
    m = m.to(DEV).bfloat16().train()
    x = torch.randint(0, 512, (2, 128), device=DEV)
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m(x)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = m(x)
        g.replay()
        a = out.clone()
        g.replay()
        b = out.clone()
        assert not torch.equal(a, b)
        assert torch.isfinite(a.float()).all() and torch.isfinite(b.float()).all()
        torch.manual_seed(3)
        e1 = m(x)
        torch.manual_seed(3)
        e2 = m(x)
        assert torch.equal(e1, e2) and not torch.equal(e1, m(x))
