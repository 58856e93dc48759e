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
* honours a ``capturable`` param-group flag: every quantity that changes from step to step is read on the device;
* keeps, with the param-group key ``ema_decay`` set (default None = off, no state key, the launches of before), an
  exponential moving average of each fp32 master in ``state[p]["ema"]``, updated by the step kernel from the new
  parameter it holds in registers: ``ema += (1 - ema_decay) * (p_new - ema)``, i.e.
  ``torch.optim.swa_utils.AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(d))`` updated once before the first step
  and once after every step.  Being optimizer state it is sharded, consolidated, checkpointed and reloaded by every
  engine like the moments; a skipped (``found_inf``) step leaves it alone.  Unlike the reference, a parameter that
  gets no gradient in a step does not advance its average in that step, and buffers are not averaged.  The key is
  read on the host at each step (fixed at capture time under graph capture, like AdamW's ``lr``).
  ``swap_ema_()`` exchanges parameters and averages in place (validation with the averaged weights) and back.
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
        self._check_ema_decay(defaults.get("ema_decay"))
        super().__init__(params, defaults)
        for group in self.param_groups:
            self._check_ema_decay(group.get("ema_decay"))
        self._tables = mt.TableCache()
        self.ema_swapped = False      # True while swap_ema_() has the averaged weights in the parameters

    # ------------------------------------------------------------------ parameter EMA
    @classmethod
    def _check_ema_decay(cls, d):
        if d is not None and not (isinstance(d, (int, float)) and 0.0 < float(d) < 1.0):
            raise ValueError(f"{cls._label}: ema_decay must be None (off) or a float in (0, 1), got {d!r}")

    def _check_not_swapped(self):
        if self.ema_swapped:
            raise RuntimeError(f"{self._label}.step(): the averaged weights are swapped in (swap_ema_); swap them "
                               "out before the next step")

    def _emas(self, group, ps):
        """-> (the fp32 averages of ``ps``, decay) for a group with ``ema_decay`` set, else (None, None).  The state
        is created here, at a parameter's first step with the average on: a clone of the fp32 master before that
        step's update, in its memory layout."""
        d = group.get("ema_decay")
        if d is None:
            return None, None
        self._check_ema_decay(d)
        emas = []
        for p in ps:
            st = self.state[p]
            e = st.get("ema")
            if e is None:
                e = st["ema"] = p.detach().clone(memory_format=torch.preserve_format)
                p._pdt_opt_state = True
            emas.append(e)
        return emas, float(d)

    @torch.no_grad()
    def swap_ema_(self) -> int:
        """Exchange every parameter that has an ``"ema"`` state with its average, in place: ONE ``swap_`` launch per
        (group, device), which also writes the bf16 compute copies (``_pdt_lp_shard``); other copies are refreshed by
        a plain copy.  The same call swaps back, bit for bit.  Call it at a step boundary; ``step()`` raises while
        ``ema_swapped`` is set.  Returns the number of parameters exchanged (0 before the first step: the average of
        a parameter that has not stepped is the parameter)."""
        n = 0
        for gi, group in enumerate(self.param_groups):
            by_dev = {}
            for p in group["params"]:
                if p in self.state and self.state[p].get("ema") is not None:
                    by_dev.setdefault(p.device, []).append(p)
            for dev, ps in by_dev.items():
                emas = [self.state[p]["ema"] for p in ps]
                lps, lp_other = self._compute_copies(ps)
                outs = lps if any(x is not None for x in lps) else None
                table = None
                if dev.type == "cuda":
                    table = self._tables.get(("swap", gi, dev), [ps, emas, outs if outs is not None else
                                                                  [None] * len(ps)])
                mt.swap_(ps, emas, outs, table=table)
                self._refresh_copies(ps, lp_other)
                n += len(ps)
        self.ema_swapped = not self.ema_swapped
        return n

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
        if self.ema_swapped:
            raise RuntimeError(f"{self._label}.load_state_dict(): swap the averaged weights out first (swap_ema_)")
        decays = [g.get("ema_decay") for g in self.param_groups]
        super().load_state_dict(state_dict)
        for g, d in zip(self.param_groups, decays):
            # torch replaces the group's keys by the checkpoint's: one written without the average (no key, or
            # off) must not switch off the average this optimizer was built with -- it starts at the next step
            if g.get("ema_decay") is None and d is not None:
                g["ema_decay"] = d
            self._check_ema_decay(g.get("ema_decay"))
        for p in self.state:
            p._pdt_opt_state = True   # engines must not re-lay-out this parameter any more (DDP rebuild)
