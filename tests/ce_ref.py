"""fp64 torch reference of the regularised cross-entropy (label smoothing eps, z-loss z), shared by the CPU and the
GPU tests of ``ops.cross_entropy(label_smoothing=, z_loss=)``:

    per non-ignored row, V = logits.shape[-1]:
      loss = lse - (1 - eps) * x[t] - (eps / V) * sum_j x[j] + z * lse^2
    ignored rows: loss 0; mean = sum over rows / number of non-ignored rows (both terms).

The gradient comes from autograd on that expression, so it is independent of the closed form the kernels use.
"""
import torch

# the project's tolerances for this op (tests/test_kernels_gpu.py::test_cross_entropy): the same roundings apply
LOSS_TOL = 2e-3                     # |loss - ref| <= LOSS_TOL * max(1, |ref|)
GRAD_TOL = {torch.bfloat16: 2e-2, torch.float32: 1e-4, torch.float16: 2e-2}    # norm-wise relative error


def rows_loss(x64, t, eps, z, ignore_index=-100):
    """Per-row loss [rows] in fp64 (0 on ignored rows); x64 is [rows, V] fp64."""
    V = x64.shape[-1]
    keep = t != ignore_index
    ts = torch.where(keep, t, torch.zeros_like(t))
    lse = torch.logsumexp(x64, -1)
    xt = x64.gather(1, ts[:, None])[:, 0]
    loss = lse - (1 - eps) * xt - (eps / V) * x64.sum(-1) + z * lse * lse
    return torch.where(keep, loss, torch.zeros_like(loss))


def reduce_loss(rows, t, reduction, ignore_index=-100):
    if reduction == "none":
        return rows
    s = rows.sum()
    return s / (t != ignore_index).sum().clamp_min(1) if reduction == "mean" else s


def ce_ref(x, t, eps=0.0, z=0.0, reduction="mean", upstream=None, ignore_index=-100):
    """(loss, grad) in fp64 for logits ``x`` [rows, V] (any float dtype: its VALUES are the inputs) and int64
    targets ``t``.  ``upstream``: the gradient fed to backward (a scalar for mean / sum, [rows] for none; 1)."""
    with torch.enable_grad():
        x64 = x.detach().double().requires_grad_()
        loss = reduce_loss(rows_loss(x64, t, eps, z, ignore_index), t, reduction, ignore_index)
        if upstream is None:
            upstream = torch.ones_like(loss)
        (grad,) = torch.autograd.grad(loss, x64, torch.as_tensor(upstream, dtype=torch.float64, device=x.device)
                                      .expand_as(loss))
    return loss.detach(), grad


def rel_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def loss_close(got, ref):
    """Element-wise |got - ref| <= LOSS_TOL * max(1, |ref|)."""
    got, ref = got.detach().double().cpu(), ref.double().cpu()
    return bool(((got - ref).abs() <= LOSS_TOL * ref.abs().clamp_min(1.0)).all())


def assert_not_vacuous(x, t, eps, z, reduction, grad_tol, upstream=None, ignore_index=-100):
    """The guard of every numeric case: the reference WITH (eps, z) differs from the plain one (eps = z = 0) by at
    least 10x the tolerance applied to the loss (element-wise on the non-ignored rows) and to the gradient
    (norm-wise), so a kernel that ignored the new terms could not pass.  Returns the reference (loss, grad)."""
    loss, grad = ce_ref(x, t, eps, z, reduction, upstream, ignore_index)
    loss0, grad0 = ce_ref(x, t, 0.0, 0.0, reduction, upstream, ignore_index)
    live = (t != ignore_index) if reduction == "none" else torch.ones((), dtype=torch.bool, device=loss.device)
    gap = (loss - loss0).abs()
    need = 10 * LOSS_TOL * loss.abs().clamp_min(1.0)
    assert bool((gap >= need)[live].all() if reduction == "none" else gap >= need), \
        ("vacuous loss check", gap.min().item(), need.max().item())
    assert rel_err(grad0, grad) >= 10 * grad_tol, ("vacuous gradient check", rel_err(grad0, grad), grad_tol)
    return loss, grad


def make_case(rows, V, dtype, device, scale=1.0, seed=0, ignore_row=3, margin=0.405):
    """Logits ``scale * randn`` in ``dtype`` with every row's target e^margin : 1 against the other columns together
    (softmax_t = 0.6 at margin log 1.5), so x[t] sits far off the row mean and the gradient's target entry, -0.4, is
    small against the one-hot: both new terms then move the loss and the gradient by far more than the tolerances,
    without softmax_t * (1 + 2 z lse) coming close to 1 (or to 1 - eps), where the gradient would be all cancellation.
    Targets include 0 and V - 1; row ``ignore_row`` is ignored (-100)."""
    g = torch.Generator(device="cpu").manual_seed(seed + V)
    x = scale * torch.randn(rows, V, generator=g, dtype=torch.float32)
    t = torch.randint(0, V, (rows,), generator=g)
    t[0], t[1] = 0, V - 1
    others = x.double().clone()
    others[torch.arange(rows), t] = float("-inf")
    x[torch.arange(rows), t] = (torch.logsumexp(others, -1) + margin).float()
    t[ignore_row] = -100
    return x.to(dtype).to(device), t.to(device)
