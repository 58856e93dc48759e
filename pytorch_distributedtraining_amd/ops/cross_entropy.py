"""Fused softmax cross-entropy over large vocabularies (gfx950 kernel, single streaming pass).

With ``inplace_backward=True`` (what the LM heads in ``models/`` pass, since their logits are dead
after the loss) the backward writes (softmax - onehot) * g IN PLACE over the saved logits, which
removes one [tokens, vocab] buffer (0.8 GB at GPT-2 1.3B / 8192 tokens per GPU).  The logits stay intact until
that backward runs.

``grad_in_forward=True`` (a separate opt-in, implies ``inplace_backward``; the LM heads pass it in training mode
only) goes one step further: where the row fits the registers of one workgroup (bf16, vocab <= 65,536: GPT-2)
and the logits require grad, the FORWARD already writes (softmax - onehot) / count over the logits in its single
read (``pdt_ce_fwd_grad``) and the backward only applies a non-unit upstream gradient: one read + one write of
the logits instead of two reads + one write.  **The logits tensor is clobbered by the forward** -- the returned
loss is correct, but any later read of the logits (or a loss taken without a backward) sees gradient values.

``label_smoothing`` (eps) and ``z_loss`` (z) are folded into the same kernels (the ``REG`` instantiations behind
``pdt_ce_reg_*``), on every path above -- a term composed around this op would read gradient values on the
``grad_in_forward`` path and cost extra passes plus an fp32 copy of the logits on the others.  Per non-ignored row,
with V = logits.shape[-1] (padded vocabulary columns included, as in torch)::

    loss   = lse - (1 - eps) * x[t] - (eps / V) * sum_j x[j] + z * lse^2
    grad_j = g * (softmax_j * (1 + 2 z lse) - (1 - eps) * [j == t] - eps / V)

Ignored rows have loss 0 and a gradient of exactly 0; ``mean`` divides both terms by the number of non-ignored
rows.  The smoothing term is ``torch.nn.functional.cross_entropy(label_smoothing=eps)``; the z term is PaLM's
``z * logsumexp(logits)^2``.  A ``-inf`` logit with ``eps > 0`` makes ``sum_j x[j]``, and so the loss, infinite, as in
torch.  At ``eps == 0 and z == 0`` the op launches exactly the plain kernels.
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from . import _lib


class _CEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, ignore_index, reduction, inplace_backward, grad_in_forward):
        V = logits.shape[-1]
        x2 = logits.reshape(-1, V)
        if x2.stride(-1) != 1:
            x2 = x2.contiguous()
        t = target.reshape(-1).to(torch.int64).contiguous()
        rows = x2.shape[0]
        loss = torch.empty(rows, dtype=torch.float32, device=logits.device)
        lse = torch.empty(rows, dtype=torch.float32, device=logits.device)
        ctx.reduction, ctx.ignore_index, ctx.inplace = reduction, ignore_index, inplace_backward
        ctx.shape = logits.shape
        ctx.eager = False
        valid = (t != ignore_index).sum().clamp_min(1).float() if reduction != "none" else None
        if (grad_in_forward and reduction != "none" and FWD_GRAD and logits.requires_grad
                and x2.dtype == torch.bfloat16 and x2.data_ptr() == logits.data_ptr()):
            # gradient written over the logits now (the row is in registers); backward applies g only
            inv = (1.0 / valid).reshape(1) if reduction == "mean" else None
            rc = _lib.require().pdt_ce_fwd_grad(x2.data_ptr(), t.data_ptr(), loss.data_ptr(), lse.data_ptr(),
                                                _lib.ptr(inv), rows, V, x2.stride(0), _lib.dtype_code(x2.dtype),
                                                int(ignore_index), _lib.stream_handle(logits.device))
            if rc == 0:
                ctx.eager = True
            elif rc != -1:
                _lib.check(rc, "pdt_ce_fwd_grad")
        if not ctx.eager:
            _lib.call("pdt_ce_fwd", x2.data_ptr(), t.data_ptr(), loss.data_ptr(), lse.data_ptr(), rows, V,
                      x2.stride(0), _lib.dtype_code(x2.dtype), int(ignore_index), _lib.stream_handle(logits.device))
        ctx.save_for_backward(x2, t, lse)
        if reduction == "none":
            return loss.view(target.shape)
        ctx.valid = valid
        s = loss.sum()
        return s / valid if reduction == "mean" else s

    @staticmethod
    def backward(ctx, g):
        x2, t, lse = ctx.saved_tensors
        rows, V = x2.shape
        if ctx.eager:   # x2 already holds (softmax - onehot) [/ count]: scale by g on the device unless g == 1
            gs = g.float().reshape(1).contiguous()
            _lib.call("pdt_ce_scale", x2.data_ptr(), gs.data_ptr(), rows, V, x2.stride(0), _lib.dtype_code(x2.dtype),
                      _lib.stream_handle(x2.device))
            return x2.view(ctx.shape), None, None, None, None, None
        grad = x2 if ctx.inplace else torch.empty_like(x2)
        if ctx.reduction == "none":
            grow = g.reshape(-1).float().contiguous()
            gscale = None
        else:
            grow = None
            gscale = (g.float() / ctx.valid).reshape(1) if ctx.reduction == "mean" else g.float().reshape(1)
        _lib.call("pdt_ce_bwd", x2.data_ptr(), t.data_ptr(), lse.data_ptr(), _lib.ptr(grow), _lib.ptr(gscale),
                  grad.data_ptr(), rows, V, x2.stride(0), grad.stride(0), _lib.dtype_code(x2.dtype),
                  int(ctx.ignore_index), _lib.stream_handle(x2.device))
        return grad.view(ctx.shape), None, None, None, None, None


# PDT_CE_FWD_GRAD=0: the two-pass forward / backward even where the fused one applies
FWD_GRAD = os.environ.get("PDT_CE_FWD_GRAD", "1") == "1"


class _CERegFn(torch.autograd.Function):
    """``_CEFn`` with label smoothing ``eps`` and z-loss ``z`` (not both zero), on the ``pdt_ce_reg_*`` entry points.
    A class of its own, so that a plain call runs ``_CEFn`` exactly as it was before the regularisers existed."""

    @staticmethod
    def forward(ctx, logits, target, ignore_index, reduction, inplace_backward, grad_in_forward, eps, z):
        V = logits.shape[-1]
        x2 = logits.reshape(-1, V)
        if x2.stride(-1) != 1:
            x2 = x2.contiguous()
        t = target.reshape(-1).to(torch.int64).contiguous()
        rows = x2.shape[0]
        loss = torch.empty(rows, dtype=torch.float32, device=logits.device)
        lse = torch.empty(rows, dtype=torch.float32, device=logits.device)
        ctx.reduction, ctx.ignore_index, ctx.inplace = reduction, ignore_index, inplace_backward
        ctx.shape, ctx.eps, ctx.z = logits.shape, eps, z
        ctx.eager = False
        valid = (t != ignore_index).sum().clamp_min(1).float() if reduction != "none" else None
        if (grad_in_forward and reduction != "none" and FWD_GRAD and logits.requires_grad
                and x2.dtype == torch.bfloat16 and x2.data_ptr() == logits.data_ptr()):
            inv = (1.0 / valid).reshape(1) if reduction == "mean" else None
            rc = _lib.require().pdt_ce_reg_fwd_grad(x2.data_ptr(), t.data_ptr(), loss.data_ptr(), lse.data_ptr(),
                                                    _lib.ptr(inv), rows, V, x2.stride(0), _lib.dtype_code(x2.dtype),
                                                    int(ignore_index), eps, z, _lib.stream_handle(logits.device))
            if rc == 0:
                ctx.eager = True
            elif rc != -1:      # -1: the row does not fit one workgroup's registers -- the two-pass kernels
                _lib.check(rc, "pdt_ce_reg_fwd_grad")
        if not ctx.eager:
            _lib.call("pdt_ce_reg_fwd", x2.data_ptr(), t.data_ptr(), loss.data_ptr(), lse.data_ptr(), rows, V,
                      x2.stride(0), _lib.dtype_code(x2.dtype), int(ignore_index), eps, z,
                      _lib.stream_handle(logits.device))
        ctx.save_for_backward(x2, t, lse)
        if reduction == "none":
            return loss.view(target.shape)
        ctx.valid = valid
        s = loss.sum()
        return s / valid if reduction == "mean" else s

    @staticmethod
    def backward(ctx, g):
        x2, t, lse = ctx.saved_tensors
        rows, V = x2.shape
        if ctx.eager:   # x2 already holds the gradient [/ count]: scale by g on the device unless g == 1
            gs = g.float().reshape(1).contiguous()
            _lib.call("pdt_ce_scale", x2.data_ptr(), gs.data_ptr(), rows, V, x2.stride(0), _lib.dtype_code(x2.dtype),
                      _lib.stream_handle(x2.device))
            return x2.view(ctx.shape), None, None, None, None, None, None, None
        grad = x2 if ctx.inplace else torch.empty_like(x2)
        if ctx.reduction == "none":
            grow = g.reshape(-1).float().contiguous()
            gscale = None
        else:
            grow = None
            gscale = (g.float() / ctx.valid).reshape(1) if ctx.reduction == "mean" else g.float().reshape(1)
        _lib.call("pdt_ce_reg_bwd", x2.data_ptr(), t.data_ptr(), lse.data_ptr(), _lib.ptr(grow), _lib.ptr(gscale),
                  grad.data_ptr(), rows, V, x2.stride(0), grad.stride(0), _lib.dtype_code(x2.dtype),
                  int(ctx.ignore_index), ctx.eps, ctx.z, _lib.stream_handle(x2.device))
        return grad.view(ctx.shape), None, None, None, None, None, None, None


def check_regularisers(label_smoothing, z_loss):
    if not 0.0 <= label_smoothing < 1.0:
        raise ValueError(f"label_smoothing must be in [0, 1), got {label_smoothing}")
    if not z_loss >= 0.0:
        raise ValueError(f"z_loss must be >= 0, got {z_loss}")


def cross_entropy(logits, target, ignore_index: int = -100, reduction: str = "mean", inplace_backward: bool = False,
                  grad_in_forward: bool = False, label_smoothing: float = 0.0, z_loss: float = 0.0):
    if label_smoothing != 0.0 or z_loss != 0.0:
        return _cross_entropy_reg(logits, target, ignore_index, reduction, inplace_backward, grad_in_forward,
                                  label_smoothing, z_loss)
    if not logits.is_cuda or logits.dtype not in (torch.float32, torch.bfloat16):
        return F.cross_entropy(logits.reshape(-1, logits.shape[-1]).float(), target.reshape(-1),
                               ignore_index=ignore_index, reduction=reduction).reshape(
            target.shape if reduction == "none" else ())
    return _CEFn.apply(logits, target, ignore_index, reduction, inplace_backward or grad_in_forward, grad_in_forward)


def _cross_entropy_reg(logits, target, ignore_index, reduction, inplace_backward, grad_in_forward, eps, z):
    check_regularisers(eps, z)
    if not logits.is_cuda or logits.dtype not in (torch.float32, torch.bfloat16):
        x, t = logits.reshape(-1, logits.shape[-1]).float(), target.reshape(-1)
        loss = F.cross_entropy(x, t, ignore_index=ignore_index, reduction=reduction, label_smoothing=eps)
        if z != 0.0:   # z * lse^2 over the non-ignored rows, reduced like the cross-entropy term
            keep = t != ignore_index
            zt = z * torch.logsumexp(x, -1).square() * keep
            if reduction == "none":
                loss = loss + zt
            else:
                loss = loss + (zt.sum() / keep.sum().clamp_min(1) if reduction == "mean" else zt.sum())
        return loss.reshape(target.shape if reduction == "none" else ())
    return _CERegFn.apply(logits, target, ignore_index, reduction, inplace_backward or grad_in_forward,
                          grad_in_forward, float(eps), float(z))


class CrossEntropyLoss(torch.nn.Module):
    """``torch.nn.CrossEntropyLoss`` drop-in on the fused kernels, plus ``z_loss``.  Class weights are not
    implemented: ``weight=`` raises."""

    def __init__(self, weight=None, ignore_index: int = -100, reduction: str = "mean", label_smoothing: float = 0.0,
                 z_loss: float = 0.0):
        super().__init__()
        if weight is not None:
            raise ValueError("CrossEntropyLoss: class weights (weight=) are not supported")
        if reduction not in ("mean", "sum", "none"):
            raise ValueError(f"reduction must be 'mean', 'sum' or 'none', got {reduction!r}")
        check_regularisers(label_smoothing, z_loss)
        self.ignore_index, self.reduction = ignore_index, reduction
        self.label_smoothing, self.z_loss = label_smoothing, z_loss

    def forward(self, logits, target):
        return cross_entropy(logits, target, ignore_index=self.ignore_index, reduction=self.reduction,
                             label_smoothing=self.label_smoothing, z_loss=self.z_loss)

    def extra_repr(self):
        return (f"ignore_index={self.ignore_index}, reduction={self.reduction!r}, "
                f"label_smoothing={self.label_smoothing}, z_loss={self.z_loss}")
