"""FusedLAMB: layer-wise adaptive moments (You et al., "Large Batch Optimization for Deep Learning"; apex
``FusedLAMB`` / timm ``Lamb`` without the clips) in two gfx950 multi-tensor launches per (param group, grad dtype).

Per logical tensor, at its step t::

    g = grad * grad_scale
    m = b1 m + (1 - b1) g ;  v = b2 v + (1 - b2) g g
    u = (m / (1 - b1^t)) / (sqrt(v) / sqrt(1 - b2^t) + eps) + wd p
    r = ||p|| / ||u||   if (wd != 0 or always_adapt) and ||p|| > 0 and ||u|| > 0, else 1
    p = p - lr r u

* The norms are taken over the WHOLE logical tensor, wherever its elements live.  An optimizer parameter may be
  something else: DDP's flat fp32 master holds every tensor of a dtype, an FSDP flat shard holds the local parts of a
  unit's tensors.  Such a parameter carries ``_pdt_segments`` (``parallel/_segments.py``): its ``spans`` become one
  table row each, and where its ``comm`` is set -- a tensor can be cut by a rank boundary -- ONE ``all_reduce(SUM)``
  of the group's ``[n_logical, 2]`` sums runs between the two stages.  A parameter without the attribute is one
  logical tensor.  OSS partitions whole parameters and needs nothing.  Alignment padding between spans belongs to no
  row: its bits never change.
* ``trust_sums[group_index]``: after a step, the ``[n_logical, 2]`` device tensor of (``||p||^2``, ``||u||^2``) of the
  group's logical tensors in parameter order (a segmented parameter contributes ``n_logical`` entries), with ``p``
  before the update -- the usual LAMB diagnostic.  A tensor without a gradient in the step reads 0.
* State, ``state_dict`` layout, device step counters, ``capturable``, ``found_inf`` / ``grad_scale``, the bf16
  compute copy and the parameter EMA: FusedAdamW's (``AdamStateOptimizer``), so a LAMB checkpoint loads into
  ``torch.optim.AdamW`` and back, and the engines shard, consolidate and checkpoint it unchanged.  A flat has its
  group's single ``weight_decay``.
* Graph capture (``capturable=True``) is supported where the step holds no collective (single process, DDP, OSS);
  with one (FSDP at world > 1, whose hooks ``Trainer.graph`` does not capture either) a captured step raises.

Stated limits (each a ValueError): ``amsgrad``, ``maximize``, a trust-ratio clip (``trust_clip``, LAMBC), an
in-optimizer ``max_grad_norm`` (clipping stays with ``optim.clip_grad_norm_`` / ``grad_scale``).  ``bias_correction``
is always on.
"""
from __future__ import annotations

import torch

from ..ops import multi_tensor as mt
from ._adam_state import AdamStateOptimizer
from ._fused import _like
from ._grads import grad_of


class FusedLAMB(AdamStateOptimizer):
    _label = "FusedLAMB"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, always_adapt=False,
                 capturable=False, ema_decay=None, amsgrad=False, maximize=False, trust_clip=False,
                 max_grad_norm=None, bias_correction=True, **_ignored):
        if amsgrad:
            raise ValueError("FusedLAMB: amsgrad is not supported")
        if maximize:
            raise ValueError("FusedLAMB: maximize is not supported")
        if trust_clip:
            raise ValueError("FusedLAMB: a trust-ratio clip (trust_clip / LAMBC) is not supported")
        if max_grad_norm is not None:
            raise ValueError("FusedLAMB: max_grad_norm is not supported; clip with optim.clip_grad_norm_ "
                             "(the step takes its device coefficient as grad_scale)")
        if not bias_correction:
            raise ValueError("FusedLAMB: bias_correction is always on")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        foreach=None, capturable=capturable, differentiable=False, fused=None,
                        always_adapt=bool(always_adapt), ema_decay=ema_decay)
        super().__init__(params, defaults)
        self.trust_sums: dict = {}      # group index -> [n_logical, 2] device tensor of (||p||^2, ||u||^2)
        self._row_views: dict = {}      # id(param) -> (key, per-span views) of a segmented parameter

    # ------------------------------------------------------------------ rows
    @staticmethod
    def _n_logical(p) -> int:
        seg = getattr(p, "_pdt_segments", None)
        return 1 if seg is None else int(seg.n_logical)

    def _rows(self, p, g, m, v, lp, e, base):
        """-> [(p, g, m, v, lp, ema, gid)] rows of one optimizer parameter: itself, or one 1-D view per span."""
        seg = getattr(p, "_pdt_segments", None)
        if seg is None:
            return [(p, g, m, v, lp, e, base)]
        tensors = (p, g, m, v, lp, e)
        key = (id(seg), len(seg.spans)) + tuple(None if t is None else (t.data_ptr(), t.numel()) for t in tensors)
        hit = self._row_views.get(id(p))
        if hit is not None and hit[0] == key:
            return hit[1]
        flat = []
        for t in tensors:
            if t is not None and not t.is_contiguous():
                raise RuntimeError("FusedLAMB: a parameter with _pdt_segments is flat (contiguous), like its state")
            flat.append(None if t is None else t.detach().view(-1))
        rows = []
        for (s, n, gid) in seg.spans:
            if not (0 <= s and 0 < n and s + n <= p.numel() and 0 <= gid < seg.n_logical):
                raise ValueError(f"FusedLAMB: span {(s, n, gid)} outside its parameter ({p.numel()} elements, "
                                 f"{seg.n_logical} logical tensors)")
            rows.append(tuple(None if t is None else t[s:s + n] for t in flat) + (base + gid,))
        self._row_views[id(p)] = (key, rows)
        return rows

    @torch.no_grad()
    def step(self, closure=None, grad_scale: torch.Tensor | None = None, found_inf: torch.Tensor | None = None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_not_swapped()
        for gi, group in enumerate(self.param_groups):
            if group.get("amsgrad", False) or group.get("maximize", False):
                raise ValueError("FusedLAMB: amsgrad / maximize are not supported")
            beta1, beta2 = group["betas"]
            lr = float(group["lr"]) if not torch.is_tensor(group["lr"]) else float(group["lr"].item())
            wd = group["weight_decay"]
            adapt = wd != 0 or bool(group.get("always_adapt", False))
            # the comms over which tensors are cut (the engine's: the same on every rank, whatever has a gradient)
            comms = {}
            for p in group["params"]:
                c = getattr(getattr(p, "_pdt_segments", None), "comm", None)
                if c is not None:
                    comms[id(c)] = c
            if comms and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
                # before anything is enqueued: the capture stays clean
                raise RuntimeError("FusedLAMB: this step all-reduces its trust-ratio sums across ranks (a sharded "
                                   "engine cuts tensors at rank boundaries) and cannot be captured into a HIP graph")
            counted = self._count_step(group, found_inf)
            if counted is None:
                continue
            buckets, counters = counted
            if not buckets:
                continue
            # logical-tensor indices: the group's parameters in order, a segmented one taking n_logical of them
            base_of, n_logical = {}, 0
            for p in group["params"]:
                base_of[id(p)] = n_logical
                n_logical += self._n_logical(p)
            dev0 = next(iter(buckets))[2]
            sums = self.trust_sums.get(gi)
            if sums is None or sums.shape[0] != n_logical or sums.device != dev0:
                sums = self.trust_sums[gi] = torch.zeros(n_logical, 2, dtype=torch.float32, device=dev0)
            else:
                sums.zero_()
            used, staged = set(), []
            for (gdt, ckey, dev), ps in buckets.items():
                if dev != dev0:
                    raise RuntimeError("FusedLAMB: the parameters of one group live on one device")
                dstep = counters.get(ckey)
                step = -ckey if dstep is None else 1
                lps, lp_other = self._compute_copies(ps)
                emas, ema_decay = self._emas(group, ps)
                rows = []
                for i, p in enumerate(ps):
                    st = self.state[p]
                    rows += self._rows(p, _like(grad_of(p), p), st["exp_avg"], st["exp_avg_sq"], lps[i],
                                       None if emas is None else emas[i], base_of[id(p)])
                cols = [list(c) for c in zip(*rows)]
                rp, rg, rm, rv, rlp, re, gids = cols
                has_lp = any(x is not None for x in rlp)
                table = row_table = ema_table = None
                if dev.type == "cuda":
                    name = (gi, gdt, ckey if dstep is not None else 0)
                    used.update((name, name + ("rows",)))
                    table = self._tables.get(name, [rp, rg, rm, rv, rlp if has_lp else [None] * len(rp)])
                    row_table = self._tables.get_rows(name + ("rows",), table, gids)
                    if emas is not None:      # the averages' pointers: a second table under a name of its own
                        used.add(name + ("ema",))
                        ema_table = self._tables.get_pointers(name + ("ema",), re, rp)
                kw = dict(beta1=beta1, beta2=beta2, eps=group["eps"], weight_decay=wd, step=max(step, 1), gids=gids,
                          found_inf=found_inf, out_bf16=rlp if has_lp else None, table=table, row_table=row_table,
                          dstep=dstep)
                mt.lamb_stage1(rp, rg, rm, rv, sums, grad_scale=grad_scale, **kw)
                staged.append((rp, rm, rv, kw, re if emas is not None else None, ema_decay, ema_table, ps, lp_other))
            for c in comms.values():      # one all-reduce of the group's sums (one comm: the engine's)
                c.all_reduce(sums, op="sum")
            for (rp, rm, rv, kw, re, ema_decay, ema_table, ps, lp_other) in staged:
                mt.lamb_stage2(rp, rm, rv, sums, lr=lr, adapt=adapt, emas=re, ema_decay=ema_decay,
                               ema_table=ema_table, **kw)
                self._refresh_copies(ps, lp_other)
            # tables of this group's counters that no longer exist (a split counter, a reloaded checkpoint)
            # are dropped, so their device tables do not pile up over a long run
            self._tables.retain(lambda n, gi=gi: n[0] != gi or n in used)
        return loss
