"""Stochastic depth on the MI355X: the scales kernel, the standalone row-scale kernel, the scaled window norm, the
scaled fused MLP and SwinIR with drop_path_rate, against torch references built with the numpy mask of
tests/dropout_ref.py or with hand-made scales (at least one dropped and one kept sample unless stated)."""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dropout_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


def rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _dp():
    return importlib.import_module("pytorch_distributedtraining_amd.ops.drop_path")


@pytest.fixture(autouse=True)
def _seed():
    torch.manual_seed(0)


def _scales(vals):
    return torch.tensor(vals, dtype=torch.float32, device=DEV)


def _rows(sc, rows_per_sample):
    """bool [B * rows_per_sample]: the rows of dropped samples."""
    return (sc == 0).repeat_interleave(rows_per_sample)


# ---- the scales kernel ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 7, 8, 9, 18])
def test_scales_kernel_matches_numpy_reference(batch):
    from test_drop_path_cpu import KEYS, RATES, ref_scales
    DP = _dp()
    keys = [k for k in KEYS for _ in RATES]
    rates = [p for _ in KEYS for p in RATES]
    got = DP.sample_scales(torch.tensor(keys, dtype=torch.int64, device=DEV), DP.site_table(rates, DEV), batch)
    assert got.is_cuda and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy(), ref_scales(keys, rates, batch))


# ---- the standalone kernel --------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("B,rps,N", [(5, 7, 3), (3, 1001, 37), (4, 64, 60)])
def test_row_scale_kernel_exact(B, rps, N, dt, with_res):
    """rows_per_sample * N = 21 and 37,037 are no multiples of the 16-byte vector (vectors straddle samples, a
    scalar tail remains), 111,111 elements take more than one workgroup; 64 x 60 is SwinIR's aligned case.
    Forward and backward against torch.where in fp32 (product and sum rounded separately, as the kernel does)."""
    from pytorch_distributedtraining_amd.ops import drop_path, drop_path_add
    sc = _scales([1.25 if b % 2 == 0 else 0.0 for b in range(B)])
    sc[-1] = 1.0 / 3.0 if B > 3 else sc[-1]
    dropped = _rows(sc, rps)
    x = torch.randn(B * rps, N, device=DEV).to(dt)
    x[dropped] = NAN                                   # never read into the result
    x.requires_grad_()
    res = torch.randn(B * rps, N, device=DEV).to(dt).requires_grad_() if with_res else None
    y = drop_path_add(res, x, sc) if with_res else drop_path(x, sc)
    dy = torch.randn_like(y)
    y.backward(dy)
    rows = sc.repeat_interleave(rps).view(-1, 1)
    zero = torch.zeros((), device=DEV)
    want = torch.where(rows != 0, x.detach().float() * rows, zero)
    if with_res:
        want = res.detach().float() + want
        assert torch.equal(res.grad, dy)
        assert torch.equal(y.detach()[dropped], res.detach()[dropped])
    assert torch.equal(y.detach(), want.to(dt))
    assert torch.equal(x.grad, torch.where(rows != 0, dy.float() * rows, zero).to(dt))
    assert 0 < int(dropped.sum()) < dropped.numel()


# ---- the scaled window norm -------------------------------------------------------------------------------------
def _win_norm_case(H, W, ws, shift, dt, sc, scaled=True, plant=True):
    from pytorch_distributedtraining_amd.models.swinir import window_partition, window_reverse
    from pytorch_distributedtraining_amd.ops.norms import (add_layer_norm_from_windows, layer_norm_to_windows,
                                                           window_norm_ok)
    torch.manual_seed(H + shift)
    B, C = 3, 60
    x = torch.randn(B, H * W, C, device=DEV, dtype=dt, requires_grad=True)
    w1, b1 = (1 + 0.1 * torch.randn(C, device=DEV)).requires_grad_(), (0.1 * torch.randn(C, device=DEV)).requires_grad_()
    w2, b2 = (1 + 0.1 * torch.randn(C, device=DEV)).requires_grad_(), (0.1 * torch.randn(C, device=DEV)).requires_grad_()
    assert window_norm_ok(x, H, W, ws, shift)
    nwin = B * (H // ws) * (W // ws)
    mix = torch.randn(C, C, device=DEV) * C ** -0.5
    win, xs = layer_norm_to_windows(x, w1, b1, 1e-5, H, W, ws, shift)
    a = (win.float() @ mix).to(dt)
    dropped = _rows(sc, H * W).view(nwin, ws * ws, 1)           # window order: a sample's windows are contiguous
    if plant:
        a = torch.where(dropped, torch.full((), NAN, device=DEV, dtype=dt), a)
    a.retain_grad()
    y, s = add_layer_norm_from_windows(xs, a, w2, b2, 1e-5, H, W, ws, shift, sample_scale=sc if scaled else None)
    gy, gs = torch.randn_like(y), torch.randn_like(s)
    (y.float() * gy.float()).sum().add_((s.float() * gs.float()).sum()).backward()
    got = dict(win=win, y=y, s=s, a_grad=a.grad, x=x, params=(w1, b1, w2, b2), gy=gy, gs=gs, mix=mix, dropped=dropped)

    xr = x.detach().float().requires_grad_()
    w1r, b1r, w2r, b2r = (t.detach().clone().requires_grad_() for t in (w1, b1, w2, b2))
    h = F.layer_norm(xr, (C,), w1r, b1r, 1e-5).view(B, H, W, C)
    winr = window_partition(torch.roll(h, (-shift, -shift), (1, 2)), ws).view(nwin, ws * ws, C)
    ar = winr @ mix
    img = torch.roll(window_reverse(ar.view(-1, ws, ws, C), ws, H, W), (shift, shift), (1, 2)).view(B, H * W, C)
    scv = sc.view(B, 1, 1)
    sr = xr + torch.where(scv != 0, img * scv, torch.zeros((), device=DEV))
    yr = F.layer_norm(sr, (C,), w2r, b2r, 1e-5)
    (yr * gy.float()).sum().add_((sr * gs.float()).sum()).backward()
    ref = dict(win=winr, y=yr, s=sr, x=xr, params=(w1r, b1r, w2r, b2r))
    return got, ref


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("H,W,ws,shift", [(32, 24, 8, 4), (16, 16, 8, 0), (14, 21, 7, 3)])
def test_scaled_window_norm_matches_fp32(H, W, ws, shift, dt):
    """test_window_mapped_norms_match_permute_path's set-up and tolerances with sample 1 dropped and samples 0 / 2
    kept at different scales; NaN fills the dropped sample's attention rows."""
    sc = _scales([1.0 / 0.9, 0.0, 2.0])
    got, ref = _win_norm_case(H, W, ws, shift, dt, sc)
    tol = 2e-2 if dt == torch.bfloat16 else 1e-5
    errs = dict(win=rel_err(got["win"], ref["win"]), s=rel_err(got["s"], ref["s"]), y=rel_err(got["y"], ref["y"]))
    gerrs = [rel_err(t.grad, r.grad) for t, r in zip((got["x"],) + got["params"], (ref["x"],) + ref["params"])]
    print(dict(H=H, W=W, ws=ws, shift=shift, dt=dt), errs, gerrs)
    assert max(errs.values()) < tol, errs
    assert max(gerrs) < 2 * tol, gerrs
    # the dropped sample: s is x's bits, its a_win gradient rows are exact zeros, and nothing anywhere is NaN
    assert torch.equal(got["s"].detach()[1], got["x"].detach()[1])
    drows = got["dropped"].expand_as(got["a_grad"])
    assert torch.equal(got["a_grad"][drows], torch.zeros_like(got["a_grad"][drows]))
    assert bool((got["a_grad"][~drows] != 0).any())
    for t in (got["y"], got["s"], got["a_grad"], got["x"].grad) + tuple(p.grad for p in got["params"]):
        assert bool(torch.isfinite(t.float()).all())


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("H,W,ws,shift", [(32, 24, 8, 4), (14, 21, 7, 3)])
def test_scaled_window_norm_at_scale_one_is_the_unscaled_kernel(H, W, ws, shift, dt):
    """(no dropped sample here, on purpose) all scales 1.0: outputs and every gradient bit-equal to today's kernels."""
    one = _scales([1.0, 1.0, 1.0])
    a, _ = _win_norm_case(H, W, ws, shift, dt, one, scaled=True, plant=False)
    b, _ = _win_norm_case(H, W, ws, shift, dt, one, scaled=False, plant=False)
    for k in ("y", "s", "a_grad"):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["x"].grad, b["x"].grad)
    for p, q in zip(a["params"], b["params"]):
        assert torch.equal(p.grad, q.grad)


# ---- the scaled fused MLP ---------------------------------------------------------------------------------------
def _mlp_weights():
    C, H = 60, 120
    w1 = (0.1 * torch.randn(H, C, device=DEV)).bfloat16().requires_grad_()
    b1 = (0.1 * torch.randn(H, device=DEV)).bfloat16().requires_grad_()
    w2 = (0.1 * torch.randn(C, H, device=DEV)).bfloat16().requires_grad_()
    b2 = (0.1 * torch.randn(C, device=DEV)).bfloat16().requires_grad_()
    return w1, b1, w2, b2


def _mlp_check(run, B, L, sc, params, plant=True):
    """``run(x, res)`` -> y on the GPU path under test; everything against fp32 torch with
    test_swin_fused_mlp_matches_fp32's tolerances.  ``plant``: NaN fills the dropped samples' x rows on the GPU
    side and the reference sees zeros there (the fused kernels never read a dropped sample's input)."""
    C = 60
    clean = torch.randn(B, L, C, device=DEV).bfloat16()
    dropped = (sc == 0)
    assert 0 < int(dropped.sum()) < B
    x = clean.clone()
    if plant:
        x[dropped] = NAN
    x.requires_grad_()
    res = torch.randn(B, L, C, device=DEV).bfloat16().requires_grad_()
    y = run(x, res)
    dy = torch.randn_like(y)
    y.backward(dy)
    xr = torch.where(dropped.view(B, 1, 1), torch.zeros((), device=DEV), clean.float()).requires_grad_()
    ref = [t.detach().float().requires_grad_() for t in params]
    branch = F.linear(F.gelu(F.linear(xr, ref[0], ref[1])), ref[2], ref[3])
    scv = sc.view(B, 1, 1)
    yr = res.detach().float() + torch.where(scv != 0, branch * scv, torch.zeros((), device=DEV))
    yr.backward(dy.float())
    errs = [rel_err(y, yr)] + [rel_err(g, w.grad) for g, w in zip([x.grad] + [p.grad for p in params], [xr] + ref)]
    print(dict(B=B, L=L), errs)
    assert errs[0] < 1e-2, errs
    assert max(errs[1:]) < 1.5e-2, errs
    assert torch.equal(y.detach()[dropped], res.detach()[dropped])            # res, bit for bit
    assert not torch.equal(y.detach()[~dropped], res.detach()[~dropped])
    assert torch.equal(x.grad[dropped], torch.zeros_like(x.grad[dropped]))    # exact zeros
    assert torch.equal(res.grad, dy)
    for t in [y] + [p.grad for p in params]:
        assert t.dtype == torch.bfloat16 and bool(torch.isfinite(t.float()).all())


@pytest.mark.parametrize("B,L,drop", [(5, 64, (1, 3)), (18, 4096, (0, 7, 17))])
def test_scaled_fused_mlp_matches_fp32(B, L, drop):
    """(5, 64): one 64-token chunk per sample, scales [s, 0, s, 0, s].  (18, 4096) = 73,728 tokens: past one grid
    pass of the forward (1,024 workgroups x 64 tokens) and of the backward (256 x 64), first and last sample
    dropped."""
    from pytorch_distributedtraining_amd.ops.swin_mlp import fused_mlp, fused_mlp_ok, fused_mlp_scaled_ok
    s = 1.0 / 0.9
    sc = _scales([0.0 if b in drop else s for b in range(B)])
    params = _mlp_weights()

    def run(x, res):
        assert fused_mlp_ok(x, *params) and fused_mlp_scaled_ok(x, res, sc)
        return fused_mlp(x, *params, res, sample_scale=sc)

    _mlp_check(run, B, L, sc, params)


def test_scaled_fused_mlp_refuses_96_token_samples_and_the_composite_serves_them():
    from pytorch_distributedtraining_amd.models.swinir import Mlp
    from pytorch_distributedtraining_amd.ops import _lib
    from pytorch_distributedtraining_amd.ops.swin_mlp import fused_mlp, fused_mlp_ok, fused_mlp_scaled_ok
    B, L, C = 4, 96, 60
    sc = _scales([1.25, 0.0, 1.25, 0.0])
    mlp = Mlp(C, 120).to(DEV).bfloat16()
    with torch.no_grad():
        for p in mlp.parameters():
            p.copy_(0.1 * torch.randn_like(p, dtype=torch.float32))
    params = (mlp.fc1.weight, mlp.fc1.bias, mlp.fc2.weight, mlp.fc2.bias)
    x = torch.randn(B, L, C, device=DEV).bfloat16()
    res = torch.randn(B, L, C, device=DEV).bfloat16()
    assert fused_mlp_ok(x, *params) and not fused_mlp_scaled_ok(x, res, sc)
    y = torch.empty_like(x)
    err = _lib.require().pdt_swin_mlp_fwd_scaled(x.data_ptr(), *(p.data_ptr() for p in params), res.data_ptr(),
                                                 y.data_ptr(), B * L, C, 120, sc.data_ptr(), L,
                                                 _lib.stream_handle(x.device))
    assert err != 0                                   # refused before any launch
    with pytest.raises(RuntimeError, match="pdt_swin_mlp_fwd_scaled"):
        fused_mlp(x, *params, res, sample_scale=sc)
    # (the composite computes the dropped samples' MLP and selects it away: no NaN planted in its input)
    _mlp_check(lambda x_, r_: mlp(x_, residual=r_, sample_scale=sc), B, L, sc, params, plant=False)


# ---- SwinIR ------------------------------------------------------------------------------------------------------
def _fixed_keys(n, device):
    """test_dropout_gpu._fixed_keys' formula."""
    return (torch.arange(n, dtype=torch.int64) * 0x0F1E2D3C4B5A6978 - 0x1234567).to(device)


def model_grad_errors(rate, dt, window_norms, monkeypatch, calls=None):
    """swinir_s_x2(depths=[2, 2], num_heads=[6, 6], drop_path_rate=rate), B = 4, 32 x 40 input, MSE loss, keys
    fixed: {parameter: relative error of its gradient on the GPU (dtype dt) against the same weights as an fp32 CPU
    model}."""
    from pytorch_distributedtraining_amd.models import swinir as S
    from pytorch_distributedtraining_amd.ops import _lib
    from pytorch_distributedtraining_amd.ops import dropout as D
    monkeypatch.setattr(D, "draw_keys", _fixed_keys)
    monkeypatch.setattr(S, "WINDOW_NORMS", window_norms)
    torch.manual_seed(0)
    kw = dict(depths=[2, 2], num_heads=[6, 6], drop_path_rate=rate)
    ref = S.swinir_s_x2(**kw).train()
    x, tgt = torch.rand(4, 3, 32, 40), torch.rand(4, 3, 64, 80)
    F.mse_loss(ref(x), tgt).backward()
    m = S.swinir_s_x2(**kw)
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).to(dt).train()
    if calls is not None:
        orig = _lib.call

        def spy(name, *a):
            calls.append(name)
            return orig(name, *a)

        monkeypatch.setattr(_lib, "call", spy)
    F.mse_loss(m(x.to(DEV).to(dt)).float(), tgt.to(DEV)).backward()
    grads = dict(ref.named_parameters())
    return {n: rel_err(p.grad.cpu(), grads[n].grad) for n, p in m.named_parameters()}


# (dtype, WINDOW_NORMS, bound): bound = 2 x the worst relative gradient error over the parameters of the same set-up
# at rate 0, where no scaled kernel and no composite pass runs (measured on an MI355X, see the docstring below)
MODEL_CASES = {
    "bf16": (torch.bfloat16, True, 2 * 7.51765e-3),
    "fp32": (torch.float32, True, 2 * 1.1192e-6),
    "bf16-no-window-norms": (torch.bfloat16, False, 2 * 7.48523e-3),
}


@pytest.mark.parametrize("case", list(MODEL_CASES))
def test_swinir_drop_path_every_grad_matches_fp32_cpu_reference(case, monkeypatch):
    """Every parameter gradient of the GPU model at drop_path_rate 0.5 against the fp32 CPU model with the same
    keys (the CPU model builds the identical per-sample masks with torch ops).  A wrong mask at any site is an O(1)
    error in the gradients upstream of it; the bound is twice the worst error of the SAME set-up at rate 0 (no
    scaled kernel runs), the margin covering the extra roundings of sc * r and sc * dy.

    Measured on one MI355X, worst relative error over the parameters (model_grad_errors):
      case                   rate 0 (unscaled paths)   bound (2 x)   rate 0.5 (this test)
      bf16                   7.51765e-3                1.50353e-2    7.43350e-3
      fp32                   1.11920e-6                2.23840e-6    1.13638e-6
      bf16-no-window-norms   7.48523e-3                1.49705e-2    7.90219e-3
    (bf16: the worst parameter is a relative_position_bias_table of the first layer at either rate.)"""
    dt, window_norms, bound = MODEL_CASES[case]
    # the condition of the test, from the numpy reference: with these keys every site keeps at least one sample and
    # at least two attention and two MLP sites drop at least one
    rates = [float(r) for r in torch.linspace(0, 0.5, 4)]
    keys = [int(k) for k in _fixed_keys(8, "cpu")]
    masks = {(k, j): R.keep_mask(4, keys[2 * k + j], rates[k]) for k in range(1, 4) for j in (0, 1)}
    assert all(m.any() for m in masks.values())
    assert sum(not masks[k, 0].all() for k in range(1, 4)) >= 2 and sum(not masks[k, 1].all() for k in range(1, 4)) >= 2
    calls = []
    errs = model_grad_errors(0.5, dt, window_norms, monkeypatch, calls)
    worst = max(errs, key=errs.get)
    print(case, "worst", worst, errs[worst], "bound", bound)
    n = {name: calls.count(name) for name in ("pdt_norm_fwd_win_scaled", "pdt_norm_bwd_win_scaled",
                                              "pdt_swin_mlp_fwd_scaled", "pdt_swin_mlp_bwd_scaled",
                                              "pdt_drop_path_rows", "pdt_drop_path_scales")}
    assert n["pdt_drop_path_scales"] == 1
    if case == "bf16":            # both scaled kernels ran at every site with a non-zero rate, no composite pass
        assert n["pdt_norm_fwd_win_scaled"] == n["pdt_norm_bwd_win_scaled"] == 3
        assert n["pdt_swin_mlp_fwd_scaled"] == n["pdt_swin_mlp_bwd_scaled"] == 3
        assert n["pdt_drop_path_rows"] == 0
    elif case == "fp32":          # the fp32 MLP is not the fused kernel's: composite around it
        assert n["pdt_norm_fwd_win_scaled"] == 3 and n["pdt_swin_mlp_fwd_scaled"] == 0
        assert n["pdt_drop_path_rows"] == 6
    else:                         # attention branch composite (forward + backward), MLP branch fused
        assert n["pdt_norm_fwd_win_scaled"] == 0 and n["pdt_swin_mlp_fwd_scaled"] == 3
        assert n["pdt_drop_path_rows"] == 6
    for name, e in errs.items():
        assert e < bound, (name, e, bound)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_swinir_drop_path_off_is_todays_model(dt, monkeypatch):
    from pytorch_distributedtraining_amd.models.swinir import swinir_s_x2
    from pytorch_distributedtraining_amd.ops import dropout as D

    def boom(n, device):
        raise AssertionError("draw_keys called with stochastic depth off")

    monkeypatch.setattr(D, "draw_keys", boom)
    torch.manual_seed(0)
    kw = dict(depths=[2, 2], num_heads=[6, 6])
    base = swinir_s_x2(**kw)
    on, zero = swinir_s_x2(drop_path_rate=0.5, **kw), swinir_s_x2(drop_path_rate=0.0, **kw)
    x = torch.rand(4, 3, 32, 40, device=DEV).to(dt)
    outs = []
    for m, train in ((base, False), (on, False), (zero, False), (base, True), (zero, True)):
        m.load_state_dict(base.state_dict())
        m = m.to(DEV).to(dt).train(train)
        with torch.no_grad():
            outs.append(m(x))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert torch.equal(outs[3], outs[4])


def test_swinir_drop_path_graph_replays_draw_fresh_keys():
    """The shape of test_gpt2_dropout_graph_replays_draw_fresh_keys: keys live in device memory and the scales
    kernel reads them there, so every replay of a captured training-mode forward drops other samples."""
    from pytorch_distributedtraining_amd.models.swinir import swinir_s_x2
    torch.manual_seed(0)
    m = swinir_s_x2(depths=[2, 2], num_heads=[6, 6], drop_path_rate=0.5).to(DEV).bfloat16().train()
    x = torch.rand(4, 3, 32, 40, device=DEV).bfloat16()
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
