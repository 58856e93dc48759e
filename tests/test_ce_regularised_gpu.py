"""Label smoothing and z-loss inside the cross-entropy kernels (MI355X): the ``REG`` instantiations behind
``pdt_ce_reg_fwd`` / ``pdt_ce_reg_bwd`` / ``pdt_ce_reg_fwd_grad`` against the fp64 reference of tests/ce_ref.py.

Tolerances are the project's own for this op (tests/test_kernels_gpu.py): loss within 2e-3 * max(1, |ref|), gradient
norm-wise 2e-2 (bf16) / 1e-4 (fp32), ignored rows exactly zero.  Every numeric case first asserts that the reference
with the new terms differs from the plain one by 10x those tolerances (``ce_ref.assert_not_vacuous``)."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import ce_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, IGN = 17, 3            # 16 live rows: 1 / count is exact in fp32
# vector path with a ragged last iteration / scalar path / fused <1024, 8> with 6,288 of 8,192 slabs live /
# fused upper bound, every slab live / two-pass, too wide for the fused kernel
VS = [1000, 50257, 50304, 65536, 128256]
BF16_REG = [(0.1, 0.0), (0.0, 1e-2), (0.1, 1e-2)]     # z = 1e-4 is invisible under the bf16 tolerances
CASES = [(torch.bfloat16, e, z) for e, z in BF16_REG] + [(torch.float32, e, z) for e, z in BF16_REG + [(0.0, 1e-4)]]


def _scale(z):
    # z = 1e-4 moves the loss by z * lse^2: logits 8x wider put lse near 40, ten times the loss tolerance again
    return 8.0 if 0 < z < 1e-3 else 1.0


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("dt,eps,z", CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_two_pass_matches_fp64_reference(V, dt, eps, z):
    """pdt_ce_reg_fwd + pdt_ce_reg_bwd: mean, sum and none (the last with a random upstream row gradient)."""
    from pytorch_distributedtraining_amd.ops import cross_entropy
    x0, t = R.make_case(ROWS, V, dt, DEV, scale=_scale(z))
    grow = torch.randn(ROWS, device=DEV, generator=torch.Generator(device=DEV).manual_seed(V)).abs() + 0.5
    for reduction, up in (("mean", None), ("sum", None), ("none", grow)):
        want, gwant = R.assert_not_vacuous(x0, t, eps, z, reduction, R.GRAD_TOL[dt], up)
        x = x0.clone().requires_grad_()
        loss = cross_entropy(x, t, reduction=reduction, label_smoothing=eps, z_loss=z)
        loss.backward(up if up is not None else None)
        err = R.rel_err(x.grad, gwant)
        print(reduction, "loss", loss.detach().double().flatten()[:2].tolist(), "ref", want.flatten()[:2].tolist(),
              "grad rel err", err)
        assert loss.shape == want.shape and R.loss_close(loss, want)
        assert err < R.GRAD_TOL[dt], err
        assert float(x.grad[IGN].float().abs().max()) == 0.0
        if reduction == "none":
            assert float(loss.detach()[IGN]) == 0.0


def _fused_case(V, reduction, gscale, eps, z, expect_fused=True):
    """The structure of test_cross_entropy_inplace_forward_gradient: ``inplace_backward`` alone leaves the logits
    bit-intact until backward; ``grad_in_forward`` returns the right loss, writes the gradient over the logits where
    the row fits one workgroup (V <= 65,536) and hands the hook the right gradient, a non-unit upstream scalar going
    through pdt_ce_scale."""
    from pytorch_distributedtraining_amd.ops import cross_entropy
    base, t = R.make_case(ROWS, V, torch.bfloat16, DEV)
    want, gwant = R.assert_not_vacuous(base, t, eps, z, reduction, R.GRAD_TOL[torch.bfloat16], gscale)
    kw = dict(reduction=reduction, label_smoothing=eps, z_loss=z)
    leaf = base.clone().requires_grad_()
    x = leaf * 1.0                                  # a non-leaf logits buffer, as a model's head output
    grads = []
    x.register_hook(grads.append)
    x0 = x.detach().clone()
    probe = cross_entropy(x, t, inplace_backward=True, **kw)          # no grad_in_forward: logits intact
    assert torch.equal(x.detach(), x0) and R.loss_close(probe, want)
    loss = cross_entropy(x, t, grad_in_forward=True, **kw)
    assert torch.equal(x.detach(), x0) != expect_fused                # the fused kernel clobbers the logits
    assert R.loss_close(loss, want), (loss.item(), want.item())
    (loss * gscale).backward()
    g = grads[0]
    err = R.rel_err(g, gwant)
    print("loss", loss.item(), "ref", want.item(), "grad rel err", err)
    assert err < R.GRAD_TOL[torch.bfloat16], err
    assert float(g[IGN].detach().float().abs().max()) == 0.0


@pytest.mark.parametrize("eps,z", BF16_REG)
@pytest.mark.parametrize("V,reduction,gscale", [(50304, "mean", 1.0), (50304, "mean", 2.5), (1000, "sum", 1.0),
                                                (65536, "sum", 0.5), (65536, "mean", 1.0), (128256, "mean", 2.5)])
def test_fused_forward_gradient(V, reduction, gscale, eps, z):
    _fused_case(V, reduction, gscale, eps, z, expect_fused=V <= 65536)


def test_fused_512x16_instantiation():
    """PDT_CE_FUSED_NTH=512 selects ce_fwd_grad_kernel<512, 16, REG> (read once per process, hence the child)."""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import test_ce_regularised_gpu as T\n"
            "T._fused_case(50304, 'mean', 2.5, 0.1, 1e-2)\nprint('fused-512 ok')\n" % (os.path.join(ROOT, "tests"), ROOT))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PDT_CE_FUSED_NTH="512"), cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fused-512 ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.parametrize("dt,V,fused", [(torch.bfloat16, 50304, True), (torch.bfloat16, 128256, False),
                                        (torch.float32, 50304, False), (torch.float32, 128256, False)],
                         ids=lambda v: str(v).replace("torch.", ""))
@pytest.mark.parametrize("eps,z", [(0.1, 0.0), (0.1, 1e-2)])
def test_uniform_term_element_for_element(dt, V, fused, eps, z):
    """The -eps / V term is far below what a norm-wise error sees.  A block of 100 non-target columns sits 40 below
    the row maximum, so softmax there is below 1e-17 and the gradient must be -(eps / V) * g element for element:
    to one bf16 rounding plus fp32 arithmetic (2^-8) in bf16, to 2^-20 in fp32.  g = 1 / 16 exactly (mean over the
    16 live rows, unit upstream gradient: no second rounding in pdt_ce_scale)."""
    from pytorch_distributedtraining_amd.ops import cross_entropy
    x0, t = R.make_case(ROWS, V, dt, DEV)
    blk = slice(128, 228)
    assert not bool(((t >= blk.start) & (t < blk.stop)).any())
    x0[:, blk] = (x0.float().max(-1, keepdim=True).values - 40.0).to(dt)
    p = torch.softmax(x0.double(), -1)[:, blk]
    assert float(p.max()) < 1e-17
    live = t != -100
    want = torch.full((ROWS, blk.stop - blk.start), -(eps / V) / int(live.sum()), dtype=torch.float64, device=DEV)
    want[~live] = 0.0
    _, gref = R.ce_ref(x0, t, eps, z)
    _, gplain = R.ce_ref(x0, t, 0.0, 0.0)
    tol = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -20
    assert bool(((gref[:, blk] - want).abs() <= 1e-9 * want.abs()).all())          # the closed form is the reference
    assert bool(((gplain[:, blk] - want).abs()[live] >= 10 * tol * want.abs()[live]).all())     # not vacuous
    leaf = x0.clone().requires_grad_()
    x = leaf * 1.0
    grads = []
    x.register_hook(grads.append)
    before = x.detach().clone()
    loss = cross_entropy(x, t, grad_in_forward=fused, label_smoothing=eps, z_loss=z)
    assert torch.equal(x.detach(), before) != fused
    loss.backward()
    got = grads[0][:, blk].double()
    worst = ((got - want).abs()[live] / want.abs()[live]).max().item()
    print("worst relative deviation from -(eps / V) * g:", worst, "allowed", tol)
    assert worst <= tol, worst
    assert float(got.detach()[~live].abs().max()) == 0.0


@pytest.mark.parametrize("V,fused", [(50304, True), (128256, False)])
def test_plain_calls_are_unchanged(V, fused, monkeypatch):
    """cross_entropy(x, t) and cross_entropy(x, t, label_smoothing=0.0, z_loss=0.0) are the same launches: no REG
    entry point is touched, and loss and gradient are bit-identical."""
    from pytorch_distributedtraining_amd.ops import _lib, cross_entropy
    lib = _lib.require()

    def boom(*a):
        raise AssertionError("a pdt_ce_reg_* entry point ran at eps = 0, z = 0")

    for name in ("pdt_ce_reg_fwd", "pdt_ce_reg_bwd", "pdt_ce_reg_fwd_grad"):
        assert getattr(lib, name) is not None
        monkeypatch.setattr(lib, name, boom)
    base, t = R.make_case(ROWS, V, torch.bfloat16, DEV)
    out = []
    for kw in ({}, dict(label_smoothing=0.0, z_loss=0.0)):
        leaf = base.clone().requires_grad_()
        x = leaf * 1.0
        loss = cross_entropy(x, t, grad_in_forward=fused, **kw)
        (loss * 1.5).backward()
        out.append((loss.detach().clone(), leaf.grad.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    want = F.cross_entropy(base.float(), t, ignore_index=-100)
    assert R.loss_close(out[0][0], want)


def _tiny(**kw):
    from pytorch_distributedtraining_amd.models import build_gpt2
    return build_gpt2("gpt2-tiny", n_embd=256, n_head=2, n_layer=2, **kw)


def test_graphed_training_step_matches_eager():
    """One GPT-2-tiny training step (vocab 512) with both terms, captured into a HIP graph and replayed, gives the
    eager step's losses (eps, eps / V and z are kernel arguments: the capture bakes them in)."""
    import copy
    from pytorch_distributedtraining_amd.optim import FusedAdamW, clip_grad_norm_
    from pytorch_distributedtraining_amd.utils.graphs import GraphedStep
    torch.manual_seed(0)
    m_eager = _tiny(label_smoothing=0.1, z_loss=1e-2).to(DEV)
    m_graph = copy.deepcopy(m_eager)
    m_plain = _tiny().to(DEV)
    m_plain.load_state_dict(m_eager.state_dict())

    def make_step(model, capturable):
        params = list(model.parameters())
        opt = FusedAdamW(params, lr=1e-3, betas=(0.9, 0.95), weight_decay=0.1, capturable=capturable)

        def step(x):
            opt.zero_grad(set_to_none=False)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = model(x[:, :-1], x[:, 1:])
            loss.backward()
            _, coef, _ = clip_grad_norm_(params, 1.0, apply=False)
            opt.step(grad_scale=coef)
            return loss.detach()
        return step

    g = torch.Generator(device=DEV).manual_seed(1)
    batches = [torch.randint(0, 512, (4, 129), device=DEV, generator=g) for _ in range(3)]
    with torch.autocast("cuda", dtype=torch.bfloat16):
        plain0 = m_plain(batches[0][:, :-1], batches[0][:, 1:]).item()
    eager = make_step(m_eager, capturable=False)
    eager_losses = [eager(batches[0]).item() for _ in range(3)]        # the graphed step's 2 warm-ups + first replay
    eager_losses += [eager(b).item() for b in batches[1:]]
    # the new terms are in the loss: far more than the tolerance away from the plain model's
    assert abs(eager_losses[0] - plain0) >= 10 * R.LOSS_TOL * max(1.0, abs(eager_losses[0])), (eager_losses[0], plain0)
    graphed = GraphedStep(make_step(m_graph, capturable=True), batches[0].clone(), warmup=2)
    graph_losses = [graphed(batches[0]).item()] + [graphed(b).item() for b in batches[1:]]
    assert graphed.eager_steps == 2
    for a, b in zip(eager_losses[2:], graph_losses):
        assert abs(a - b) < R.LOSS_TOL * max(1.0, abs(a)), (eager_losses, graph_losses)


def test_gpt2_matches_fp32_cpu_model_and_eval_is_plain():
    """GPT-2-tiny in bf16 on the HIP kernels, training forward + backward with both terms, against the same model in
    fp32 on the CPU (the op's torch fallback computes the same definition): loss, and the tied embedding's gradient
    at the model-level tolerance of tests/test_dropout_gpu.py (4e-2 norm-wise).  eps = 0.5, z = 0.1 so that the
    reference moves by 10x those tolerances.  In eval() the same model returns plain cross-entropy."""
    eps, z = 0.5, 0.1
    torch.manual_seed(0)
    ref = _tiny(label_smoothing=eps, z_loss=z)
    plain = _tiny()
    plain.load_state_dict(ref.state_dict())
    x = torch.randint(0, 512, (4, 129))
    lr = ref(x[:, :-1], labels=x[:, 1:])
    lr.backward()
    lp = plain(x[:, :-1], labels=x[:, 1:])
    lp.backward()
    assert abs(lr.item() - lp.item()) >= 10 * R.LOSS_TOL * max(1.0, abs(lr.item()))
    assert R.rel_err(plain.wte.weight.grad, ref.wte.weight.grad) >= 10 * 4e-2
    m = _tiny(label_smoothing=eps, z_loss=z)
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).bfloat16()
    xd = x.to(DEV)
    loss = m(xd[:, :-1], labels=xd[:, 1:])
    loss.backward()
    err = R.rel_err(m.wte.weight.grad.cpu(), ref.wte.weight.grad)
    print("loss", loss.item(), "ref", lr.item(), "wte grad rel err", err)
    assert R.loss_close(loss, lr.detach()), (loss.item(), lr.item())
    assert err < 4e-2, err
    m.eval()
    with torch.no_grad():
        le = m(xd[:, :-1], labels=xd[:, 1:])
        logits = m(xd[:, :-1])
    want = F.cross_entropy(logits.float().reshape(-1, logits.shape[-1]), xd[:, 1:].reshape(-1))
    assert R.loss_close(le, want), (le.item(), want.item())
    assert abs(le.item() - loss.item()) >= 10 * R.LOSS_TOL * max(1.0, abs(le.item()))
