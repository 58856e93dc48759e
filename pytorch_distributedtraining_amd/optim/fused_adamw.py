"""FusedAdamW: torch.optim-compatible AdamW whose step is ONE gfx950 multi-tensor launch per
(param group, grad dtype).

* ``param_groups`` / ``state_dict`` layout identical to torch.optim.AdamW
  ({state: {idx: {step, exp_avg, exp_avg_sq}}, param_groups: [...]}, torch/optim/optimizer.py:677-760),
  so LR schedulers (OneCycleLR cycling betas, Stoke-DDP.py:300) and checkpoints interoperate.
* Sync-free mixed precision: ``step(grad_scale=t, found_inf=f)`` takes device scalars produced by the
  fused clip / unscale kernels; no host round trip between backward and the update.
* fp16 overflow: a step whose ``found_inf`` flag is set changes nothing -- parameters, moments and the
  step count (torch.amp.GradScaler skips ``optimizer.step()``, grad_scaler.py:360); the device count
  advances only when the flag is clear.
* Graph capture (``capturable=True``): the step count of each param group lives in a device tensor that a
  captured kernel increments, and the AdamW kernel derives its bias corrections from it, so a training step
  captured into a HIP graph (``utils.graphs.GraphedStep``) replays with the right step every time.  The
  learning rate is read when the step is captured (a schedule needs a re-capture).
* Parameter EMA (``ema_decay``, a param-group key, default None = off): ``state[p]["ema"]``, updated by the same
  launch -- see ``FusedOptimizer``.  The state layout is torch's plus that key, which torch.optim.AdamW carries.
* Sharded engines: a parameter carrying ``_pdt_lp_shard`` (FSDP / ZeRO flat shards) gets its bf16
  compute copy written by the same kernel (fused cast epilogue = the all-gather input).

Reference: AdamW(lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-4) in Stoke-DDP.py:226-235
and Fairscale-DDP.py:78-86; math order torch/optim/adam.py:419-547.
"""
from __future__ import annotations

import torch

from ..ops import multi_tensor as mt
from ._adam_state import AdamStateOptimizer
from ._fused import FusedOptimizer, _like, _same_layout  # noqa: F401
from ._grads import grad_of


class FusedAdamW(AdamStateOptimizer):
    _label = "FusedAdamW"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False,
                 decoupled=True, capturable=False, ema_decay=None, **_ignored):
        if amsgrad:
            raise ValueError("FusedAdamW: amsgrad is not supported")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False,
                        maximize=False, foreach=None, capturable=capturable, differentiable=False, fused=None,
                        decoupled=decoupled, ema_decay=ema_decay)
        super().__init__(params, defaults)

    @torch.no_grad()
    def step(self, closure=None, grad_scale: torch.Tensor | None = None, found_inf: torch.Tensor | None = None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_not_swapped()
        for gi, group in enumerate(self.param_groups):
            beta1, beta2 = group["betas"]
            lr = float(group["lr"]) if not torch.is_tensor(group["lr"]) else float(group["lr"].item())
            counted = self._count_step(group, found_inf)
            if counted is None:
                continue
            buckets, counters = counted
            used = set()
            for (gdt, ckey, dev), ps in buckets.items():
                dstep = counters.get(ckey)
                step = -ckey if dstep is None else 1
                grads = [_like(grad_of(p), p) for p in ps]
                ms = [self.state[p]["exp_avg"] for p in ps]
                vs = [self.state[p]["exp_avg_sq"] for p in ps]
                lps, lp_other = self._compute_copies(ps)
                has_lp = any(x is not None for x in lps)
                emas, ema_decay = self._emas(group, ps)
                table = ema_table = None
                if dev.type == "cuda":
                    cols = [ps, grads, ms, vs, lps if has_lp else [None] * len(ps)]
                    name = (gi, gdt, ckey if dstep is not None else 0)
                    used.add(name)
                    table = self._tables.get(name, cols)
                    if emas is not None:      # the averages' pointers: a second table under a name of its own
                        used.add(name + ("ema",))
                        ema_table = self._tables.get_pointers(name + ("ema",), emas, ps)
                mt.adamw_step(ps, grads, ms, vs, lr=lr, beta1=beta1, beta2=beta2, eps=group["eps"],
                              weight_decay=group["weight_decay"], step=max(step, 1),
                              decoupled=group.get("decoupled", True), grad_scale=grad_scale, found_inf=found_inf,
                              out_bf16=lps if has_lp else None, table=table, dstep=dstep, emas=emas,
                              ema_decay=ema_decay, ema_table=ema_table)
                self._refresh_copies(ps, lp_other)
            if buckets:
                # tables of this group's counters that no longer exist (a split counter, a reloaded checkpoint)
                # are dropped, so their device tables do not pile up over a long run
                self._tables.retain(lambda n, gi=gi: n[0] != gi or n in used)
        return loss
