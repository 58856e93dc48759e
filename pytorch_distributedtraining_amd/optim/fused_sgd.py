"""FusedSGD: torch.optim-compatible SGD (momentum / Nesterov, L2 weight decay) whose step is ONE gfx950
multi-tensor launch per (param group, grad dtype, device).

* ``param_groups`` keys and ``state_dict`` layout are torch.optim.SGD's ({state: {idx: {momentum_buffer}}},
  no state at all with momentum 0), so LR schedulers and checkpoints move both ways.  A loaded
  ``momentum_buffer`` of None counts as zeros.
* Math order of torch/optim/sgd.py ``_single_tensor_sgd`` with dampening 0.  The momentum buffer starts at zero,
  which reproduces torch's first step (``buf = clone(g)`` equals ``momentum * 0 + g``): the kernel needs no notion
  of a first step, a skipped (``found_inf``) step changes nothing at all, and graph capture needs nothing extra.
* Learning-rate schedules under graph capture: a ``group["lr"]`` that is a tensor on the parameters' device is read
  by the kernel from the device (no ``.item()``), so a captured step follows a scheduler that ``fill_``s it in place
  (torch/optim/lr_scheduler.py ``_update_param_group_val``).  A float is passed by value, i.e. read at capture.
* Sync-free mixed precision, sharded engines' bf16 compute copies, the parameter EMA (``ema_decay``, a param-group
  key beyond torch's, default None = off; ``state[p]["ema"]``): as ``FusedOptimizer`` describes.

Stated limits (each raises): ``dampening != 0``, ``maximize=True``, Nesterov without momentum (torch's own rule)
are ValueErrors; sparse gradients a RuntimeError; non-fp32 parameters a TypeError.
"""
from __future__ import annotations

import torch

from ..ops import multi_tensor as mt
from ._fused import FusedOptimizer, _like
from ._grads import grad_of


class FusedSGD(FusedOptimizer):
    _label = "FusedSGD"

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False,
                 capturable=False, ema_decay=None, **_ignored):
        if dampening != 0:
            raise ValueError("FusedSGD: dampening is not supported")
        if maximize:
            raise ValueError("FusedSGD: maximize is not supported")
        if nesterov and momentum <= 0:
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        if momentum < 0 or weight_decay < 0:
            raise ValueError(f"FusedSGD: invalid momentum {momentum} / weight_decay {weight_decay}")
        defaults = dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=False, foreach=None, differentiable=False, fused=None)
        if ema_decay is not None:      # the one key beyond torch's, stored only when set: off, the groups are torch's
            defaults["ema_decay"] = ema_decay
        # ``capturable`` is accepted for symmetry with FusedAdamW and not stored (the group keys stay torch's):
        # SGD keeps no step count, so every step is capturable as it is
        super().__init__(params, defaults)

    def _buffer(self, p):
        st = self.state[p]
        if st.get("momentum_buffer") is None:      # new state, or torch's None (saved before any step)
            st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format, dtype=torch.float32)
            p._pdt_opt_state = True
        return st["momentum_buffer"]

    @torch.no_grad()
    def step(self, closure=None, grad_scale: torch.Tensor | None = None, found_inf: torch.Tensor | None = None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_not_swapped()
        for gi, group in enumerate(self.param_groups):
            if group.get("dampening", 0) != 0 or group.get("maximize", False):
                raise ValueError("FusedSGD: dampening / maximize are not supported")
            momentum, nesterov = group["momentum"], bool(group["nesterov"])
            if nesterov and momentum <= 0:
                raise ValueError("Nesterov momentum requires a momentum and zero dampening")
            if found_inf is not None and found_inf.device.type != "cuda" and int(found_inf.reshape(-1)[0]) != 0:
                continue        # a host flag: the skipped step launches nothing
            buckets = {}
            for p in self._present(group):
                buckets.setdefault((grad_of(p).dtype, p.device), []).append(p)
            for (gdt, dev), ps in buckets.items():
                lr = group["lr"]
                if torch.is_tensor(lr) and not (dev.type == "cuda" and lr.device == dev):
                    lr = float(lr)        # a host tensor (torch allows one): by value
                grads = [_like(grad_of(p), p) for p in ps]
                bufs = [self._buffer(p) for p in ps] if momentum != 0 else None
                lps, lp_other = self._compute_copies(ps)
                has_lp = any(x is not None for x in lps)
                emas, ema_decay = self._emas(group, ps)
                table = ema_table = None
                if dev.type == "cuda":
                    none = [None] * len(ps)
                    table = self._tables.get((gi, gdt, dev), [ps, grads, bufs if bufs is not None else none, none,
                                                              lps if has_lp else none])
                    if emas is not None:      # the averages' pointers: a second table under a name of its own
                        ema_table = self._tables.get_pointers((gi, gdt, dev, "ema"), emas, ps)
                mt.sgd_step(ps, grads, bufs, lr=lr, momentum=momentum, weight_decay=group["weight_decay"],
                            nesterov=nesterov, grad_scale=grad_scale, found_inf=found_inf,
                            out_bf16=lps if has_lp else None, table=table, emas=emas, ema_decay=ema_decay,
                            ema_table=ema_table)
                self._refresh_copies(ps, lp_other)
        return loss
