"""FusedOptimizer: what the framework's multi-tensor optimizers share, and the class the engines and the
Trainer test for when they switch on their fast paths.

A FusedOptimizer
* steps fp32 master parameters with ONE gfx950 multi-tensor launch per (param group, grad dtype, device), through a
  ``TableCache`` of device tensor tables (``ops/multi_tensor.py``);
* reads gradients through ``grad_of`` (an engine's low-precision flat gradient, or a master's module parameter);
* ``step(closure=None, grad_scale=None, found_inf=None)`` takes the device scalars of the fused clip / unscale
  kernels, so no host round trip sits between backward and the update, and a set ``found_inf`` changes nothing;
* writes the bf16 compute copy ``_pdt_lp_shard`` of a parameter in the kernel's epilogue (a non-bf16 copy is
  refreshed by a plain copy) and records it in ``_pdt_lp_version``;
* honours a ``capturable`` param-group flag: every quantity that changes from step to step is read on the device.
"""
from __future__ import annotations

import torch
from torch.optim import Optimizer

from ..ops import multi_tensor as mt
from ..ops.multi_tensor import _dense
from ._grads import grad_of


def _same_layout(g, p) -> bool:
    """Same element order in memory: strides equal wherever the size is not 1 (a size-1 dimension's stride is
    arbitrary -- a contiguous [Cout, Cin, 1, 1] gradient of a channels_last 1x1-conv weight is already in its order,
    and autograd's layout contract accepts it as is)."""
    return g.shape == p.shape and all(gs == ps for gs, ps, n in zip(g.stride(), p.stride(), p.shape) if n != 1)


def _like(g, p):
    """The gradient in the parameter's memory layout (the kernel walks storage linearly)."""
    if p.dim() <= 1:
        return g if g.is_contiguous() else g.contiguous()
    if _same_layout(g, p) and _dense(g):
        return g
    return torch.empty_like(p, dtype=g.dtype).copy_(g)


class FusedOptimizer(Optimizer):
    _label = "FusedOptimizer"     # the public name error messages use

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._tables = mt.TableCache()

    def _present(self, group):
        """The group's parameters that have a gradient this step (fp32 masters with dense gradients only)."""
        name = self._label
        present = []
        for p in group["params"]:
            g = grad_of(p)
            if g is None:
                continue
            if g.is_sparse:
                raise RuntimeError(f"{name} does not support sparse gradients")
            if p.dtype != torch.float32:
                raise TypeError(f"{name} keeps fp32 master params; wrap low-precision models with an "
                                "engine (FSDP/ZeRO) or keep params fp32 and use autocast")
            present.append(p)
        return present

    @staticmethod
    def _compute_copies(ps):
        """-> (bf16 copies for the kernel's epilogue, or None where there is none; [(param, non-bf16 copy)]).

        The kernel's epilogue writes bf16 compute copies; an fp32 "copy" (a DDP compute-copy model's batch-norm
        group) is refreshed by a plain copy after the step (``_refresh_copies``)."""
        lps = [getattr(p, "_pdt_lp_shard", None) for p in ps]
        other = [(p, x) for p, x in zip(ps, lps) if x is not None and x.dtype != torch.bfloat16]
        return [x if (x is not None and x.dtype == torch.bfloat16) else None for x in lps], other

    @staticmethod
    def _refresh_copies(ps, other):
        with torch.no_grad():
            for p, x in other:
                x.copy_(p)
        for p in ps:
            if getattr(p, "_pdt_lp_shard", None) is not None:
                p._pdt_lp_version = p._version   # compute copy already refreshed by the kernel

    def zero_grad(self, set_to_none: bool = True):
        """torch semantics for ``.grad``, except for engine-owned flat gradients: DDP's compute-dtype masters
        (``_pdt_zero_grad``) and parameters whose ``.grad`` is still a view of a DDP bucket flat
        (``_pdt_grad_flat``) get their flat zeroed in place -- ONE fill per flat instead of a None per
        parameter that the next forward would re-attach view by view (ResNet-50: 161 views, a host gap at
        every step start).  Those gradients therefore read as zeros, not None, after ``set_to_none=True`` (as
        with torch DDP's ``gradient_as_bucket_view``, whose views stay attached to the bucket).  A flat is filled
        whole only when every parameter viewing it (``_pdt_grad_members``) belongs to THIS optimizer; otherwise
        only this optimizer's own views are zeroed, so another optimizer stepping the same bucket later still
        sees its gradients."""
        mine = {id(p) for group in self.param_groups for p in group["params"]}
        flats, views, rest, owned = {}, [], [], {}
        for group in self.param_groups:
            for p in group["params"]:
                zero = getattr(p, "_pdt_zero_grad", None)
                if zero is not None:
                    flats[id(zero)] = zero
                    continue
                g = p.grad
                if g is None:
                    continue
                f = getattr(p, "_pdt_grad_flat", None)
                if f is not None and g._base is f:
                    ok = owned.get(id(f))
                    if ok is None:
                        members = getattr(p, "_pdt_grad_members", None)
                        ok = owned[id(f)] = members is not None and all(id(q) in mine for q in members)
                    if ok:
                        flats[id(f)] = f.zero_
                    else:
                        views.append(g)      # keep the view attached: the bucket reduction reads it in place
                    continue
                rest.append(p)
        for zero in flats.values():
            if getattr(zero, "_pdt_set_to_none", False):
                zero(set_to_none)      # an engine that keeps per-parameter gradients (DDP._steal_grads)
            else:
                zero()
        if views:
            torch._foreach_zero_(views)
        if set_to_none:
            for p in rest:
                p.grad = None
        elif rest:
            grads = []
            for p in rest:
                if p.grad.grad_fn is not None:
                    p.grad.detach_()
                else:
                    p.grad.requires_grad_(False)
                grads.append(p.grad)
            torch._foreach_zero_(grads)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for p in self.state:
            p._pdt_opt_state = True   # engines must not re-lay-out this parameter any more (DDP rebuild)
