"""Multi-tensor launches: fused AdamW, fused SGD, two-stage fused LAMB, fused L2 norm (+ non-finite check), clip coefficient, scale.

One HIP launch covers an arbitrary list of tensors through a device-resident table
(``csrc/kernels/multi_tensor.hip``).  The engines keep parameters/gradients in flat buffers so their
tables have a single entry; user parameter lists get one table per (dtype, group).

Reference parity: AdamW as configured in Stoke-DDP.py:226-235 / Fairscale-DDP.py:78-86 (math order
of torch/optim/adam.py:419-547), clip_grad_norm_ as configured by Stoke-DDP.py:253
(torch/nn/utils/clip_grad.py:50-186).
"""
from __future__ import annotations

import math
from typing import Sequence

import torch

from . import _lib

META = 6
DEFAULT_CHUNK = 32768


def _dense(t: torch.Tensor) -> bool:
    return t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last)) or \
        (t.dim() == 5 and t.is_contiguous(memory_format=torch.channels_last_3d))


class TensorTable:
    """Device table describing up to 5 aligned tensor lists (+ numel) for a multi-tensor kernel.

    ``cols`` is a list of columns, each a list of tensors (or None) of equal length; column 0 defines
    the numel.  The table holds raw pointers, so the caller must keep the tensors alive and must
    rebuild the table if any storage is reallocated (``key()`` changes).
    """

    def __init__(self, cols: Sequence[Sequence[torch.Tensor | None]], chunk: int = DEFAULT_CHUNK):
        assert 1 <= len(cols) <= 5
        n = len(cols[0])
        for c in cols:
            assert len(c) == n
        self.chunk = int(chunk)
        self.cols = [list(c) for c in cols]
        self.numels = [t.numel() for t in cols[0]]
        dev = cols[0][0].device if n else torch.device("cpu")
        rows = max(n, 1)
        counts = torch.tensor([(m + self.chunk - 1) // self.chunk for m in self.numels] or [0], dtype=torch.int64)
        self.nblocks = int(counts.sum())
        nb = max(self.nblocks, 1)
        # ONE host buffer = meta rows (int64) followed by the (tensor, chunk) int32 pairs packed two per int64
        # word, filled without a per-chunk Python loop and uploaded with ONE asynchronous copy from pinned
        # memory: a pageable copy blocks the host until the stream drains (the whole backward, before the
        # clip norm) and the per-chunk loop cost ~4 ms per 1.3B-parameter table -- both idle GPU time
        # (profiles/r3_s4g_gpt2_1.3b_fsdp1_mb96_kernel_table.txt).
        host = torch.zeros(rows * META + nb, dtype=torch.int64, pin_memory=dev.type == "cuda")
        meta = host[:rows * META].view(rows, META)
        for i in range(n):
            ref = cols[0][i]
            for j, col in enumerate(cols):
                t = col[i]
                if t is not None:
                    # elementwise over the storage: any dense layout works if every column shares it
                    assert _dense(t), "multi-tensor kernels need dense (non-overlapping) tensors"
                    assert t.numel() == self.numels[i]
                    assert t.dim() <= 1 or all(a == b for a, b, k in zip(t.stride(), ref.stride(), ref.shape) if k != 1), \
                        "multi-tensor columns must share a layout"   # (a size-1 dimension's stride is arbitrary)
                    meta[i, j] = t.data_ptr()
            meta[i, 5] = self.numels[i]
        if self.nblocks:
            tid = torch.repeat_interleave(torch.arange(len(counts), dtype=torch.int64), counts)
            first = torch.cumsum(counts, 0) - counts
            cid = torch.arange(self.nblocks, dtype=torch.int64) - torch.repeat_interleave(first, counts)
            host[rows * META:] = tid | (cid << 32)           # little-endian: int32 pair (tensor, chunk)
        if dev.type == "cuda":
            buf = host.to(dev, non_blocking=True)
            self._host = host                                 # pinned source stays alive with the table
        else:
            buf = host
        self.meta = buf[:rows * META].view(rows, META)
        self.blk = buf[rows * META:].view(torch.int32).view(nb, 2)
        self._key = self.make_key(cols)
        self.device = dev

    @staticmethod
    def make_key(cols) -> tuple:
        return tuple((t.data_ptr(), t.numel()) if t is not None else None for c in cols for t in c)

    def key(self) -> tuple:
        return self._key


class PointerTable:
    """One device pointer per row (null where the row has none), in the row order of the ``TensorTable`` it goes with:
    the second table of the parameter-EMA step kernels (the 6-word row has no free column under AdamW)."""

    def __init__(self, tensors: Sequence[torch.Tensor | None], like: Sequence[torch.Tensor]):
        assert len(tensors) == len(like)
        dev = like[0].device if len(like) else torch.device("cpu")
        host = torch.zeros(max(len(tensors), 1), dtype=torch.int64, pin_memory=dev.type == "cuda")
        for i, (t, ref) in enumerate(zip(tensors, like)):
            if t is not None:
                assert t.dtype == torch.float32 and t.device == ref.device and t.numel() == ref.numel()
                assert _dense(t) and (t.dim() <= 1 or all(
                    a == b for a, b, k in zip(t.stride(), ref.stride(), ref.shape) if k != 1)), \
                    "the parameter average must share its parameter's memory layout"
                host[i] = t.data_ptr()
        if dev.type == "cuda":
            self.ptrs = host.to(dev, non_blocking=True)
            self._host = host                                 # pinned source stays alive with the table
        else:
            self.ptrs = host
        self._key = TensorTable.make_key([tensors])

    def key(self) -> tuple:
        return self._key


class RowTable:
    """Three int32 words per row of a ``TensorTable`` -- [first block, block count, logical-tensor index] -- for the
    LAMB kernels: a row's blocks are consecutive in the block table, so its per-block partial sums are one span, and
    ``gids[row]`` names the logical tensor whose norms the row adds to (a row is a whole tensor or the local part of
    one).  A logical tensor sits on at most one row."""

    def __init__(self, table: TensorTable, gids: Sequence[int]):
        gids = [int(g) for g in gids]
        assert len(gids) == len(table.numels)
        assert len(set(gids)) == len(gids), "a logical tensor may sit on one table row only"
        n = len(gids)
        dev = table.device
        host = torch.zeros(max(n, 1), 3, dtype=torch.int32, pin_memory=dev.type == "cuda")
        if n:
            counts = torch.tensor([(m + table.chunk - 1) // table.chunk for m in table.numels], dtype=torch.int64)
            host[:, 0] = (torch.cumsum(counts, 0) - counts).to(torch.int32)
            host[:, 1] = counts.to(torch.int32)
            host[:, 2] = torch.tensor(gids, dtype=torch.int32)
        if dev.type == "cuda":
            self.rows = host.to(dev, non_blocking=True)
            self._host = host                                 # pinned source stays alive with the table
        else:
            self.rows = host
        self.nrows = n
        self.gids = gids
        self.max_gid = max(gids) if gids else -1
        self._key = (table.key(), tuple(gids))

    def key(self) -> tuple:
        return self._key


class TableCache:
    """Rebuilds a TensorTable only when the pointer set changes."""

    def __init__(self):
        self._tables = {}

    def get_rows(self, name, table: TensorTable, gids) -> RowTable:
        t = self._tables.get(name)
        if t is None or t.key() != (table.key(), tuple(gids)):
            t = RowTable(table, gids)
            self._tables[name] = t
        return t

    def get_pointers(self, name, tensors, like) -> PointerTable:
        key = TensorTable.make_key([tensors])
        t = self._tables.get(name)
        if t is None or t.key() != key:
            t = PointerTable(tensors, like)
            self._tables[name] = t
        return t

    def get(self, name, cols, chunk=DEFAULT_CHUNK) -> TensorTable:
        key = TensorTable.make_key(cols)
        t = self._tables.get(name)
        if t is None or t.key() != key:
            t = TensorTable(cols, chunk)
            self._tables[name] = t
        return t

    def retain(self, keep) -> None:
        """Drop every cached table whose name fails ``keep(name)`` (its device table is freed with it)."""
        for n in [n for n in self._tables if not keep(n)]:
            del self._tables[n]

    def __len__(self):
        return len(self._tables)


_cache = TableCache()


def l2norm_sq(tensors: Sequence[torch.Tensor], out: torch.Tensor | None = None, accumulate=False,
              table: TensorTable | None = None) -> torch.Tensor:
    """Sum of squares over all tensors as a 1-element fp32 device tensor (no host sync)."""
    tensors = [t for t in tensors if t is not None and t.numel() > 0]
    if not tensors:
        o = out if out is not None else torch.zeros(1, dtype=torch.float32)
        if not accumulate:
            o.zero_()
        return o
    dev = tensors[0].device
    if out is None:
        out = torch.zeros(1, dtype=torch.float32, device=dev)
    if dev.type != "cuda":
        s = torch.zeros((), dtype=torch.float32)
        for t in tensors:
            s = s + t.detach().float().pow(2).sum()
        if accumulate:
            out.add_(s)
        else:
            out.copy_(s.reshape(1))
        return out
    by_dt = {}
    for t in tensors:
        by_dt.setdefault(t.dtype, []).append(t)
    first = True
    for dt, ts in by_dt.items():
        tab = table if (table is not None and len(by_dt) == 1) else _cache.get(("l2", dt, len(ts)), [ts])
        partial = torch.empty(max(tab.nblocks, 1), dtype=torch.float32, device=dev)
        _lib.call("pdt_l2norm_mt", tab.meta.data_ptr(), tab.blk.data_ptr(), tab.nblocks, tab.chunk,
                  _lib.dtype_code(dt), partial.data_ptr(), out.data_ptr(), 1 if (accumulate or not first) else 0,
                  _lib.stream_handle(dev))
        first = False
    return out


def clip_coef(total_sq: torch.Tensor, max_norm: float, inv_scale: torch.Tensor | float = 1.0):
    """From an (all-reduced) sum of squares: (norm, grad_multiplier, found_inf) device tensors.

    grad_multiplier = min(1, max_norm/(norm+1e-6)) * inv_scale; max_norm<=0 disables clipping."""
    dev = total_sq.device
    norm = torch.empty(1, dtype=torch.float32, device=dev)
    coef = torch.empty(1, dtype=torch.float32, device=dev)
    found = torch.empty(1, dtype=torch.int32, device=dev)
    if dev.type != "cuda":
        inv = float(inv_scale) if not torch.is_tensor(inv_scale) else float(inv_scale.reshape(-1)[0])
        sq = float(total_sq.reshape(-1)[0])
        fin = math.isfinite(sq)
        nrm = math.sqrt(sq) * inv if fin else float("nan") if sq != sq else float("inf")
        c = min(max_norm / (nrm + 1e-6), 1.0) if (max_norm > 0 and fin) else 1.0
        norm.fill_(nrm)
        coef.fill_(c * inv)
        found.fill_(0 if fin else 1)
        return norm, coef, found
    if torch.is_tensor(inv_scale):
        inv_ptr, inv_val = inv_scale.data_ptr(), 1.0
    else:
        inv_ptr, inv_val = 0, float(inv_scale)
    _lib.call("pdt_clip_coef", total_sq.data_ptr(), float(max_norm), inv_ptr, inv_val, norm.data_ptr(),
              coef.data_ptr(), found.data_ptr(), _lib.stream_handle(dev))
    return norm, coef, found


def scale_(tensors: Sequence[torch.Tensor], s: torch.Tensor) -> None:
    """In-place multiply every tensor by the device scalar ``s``."""
    tensors = [t for t in tensors if t is not None and t.numel() > 0]
    if not tensors:
        return
    dev = tensors[0].device
    if dev.type != "cuda":
        for t in tensors:
            t.mul_(s.to(t.dtype))
        return
    by_dt = {}
    for t in tensors:
        by_dt.setdefault(t.dtype, []).append(t)
    for dt, ts in by_dt.items():
        tab = _cache.get(("scale", dt, len(ts)), [ts])
        _lib.call("pdt_scale_mt", tab.meta.data_ptr(), tab.blk.data_ptr(), tab.nblocks, tab.chunk,
                  _lib.dtype_code(dt), s.data_ptr(), _lib.stream_handle(dev))


def _ema_weight(emas, ema_decay, who: str, rows: int):
    """-> ``w = 1 - decay`` (computed in double, rounded to fp32 where it is used), or None when the average is off."""
    if emas is None and ema_decay is None:
        return None
    if emas is None or ema_decay is None:
        raise ValueError(f"{who}: emas and ema_decay go together")
    d = float(ema_decay)
    if not 0.0 < d < 1.0:
        raise ValueError(f"{who}: ema_decay must be in (0, 1), got {ema_decay}")
    if len(emas) != rows:
        raise ValueError(f"{who}: {len(emas)} averages for {rows} parameters (None where a parameter keeps none)")
    return 1.0 - d


def _ema_cpu_(e: torch.Tensor, p: torch.Tensor, w: float) -> None:
    """ema <- ema + w * (p - ema) in fp32 (the kernels' formula; torch's lerp for w < 0.5)."""
    e.add_(p - e, alpha=float(torch.tensor(w, dtype=torch.float32)))


def adamw_step(params, grads, exp_avgs, exp_avg_sqs, *, lr: float, beta1: float, beta2: float, eps: float,
               weight_decay: float, step: int, decoupled: bool = True, grad_scale: torch.Tensor | None = None,
               found_inf: torch.Tensor | None = None, out_bf16=None, table: TensorTable | None = None,
               dstep: torch.Tensor | None = None, emas=None, ema_decay: float | None = None,
               ema_table: PointerTable | None = None) -> None:
    """One fused (multi-tensor) AdamW update.  fp32 params/state; grads fp32 or bf16.

    grad_scale: optional device scalar multiplied into every gradient (unscale x clip coefficient).
    found_inf: optional device int32 flag; non-zero skips the update (GradScaler semantics).
    out_bf16: optional list of bf16 tensors receiving the updated params (low-precision compute copy /
    all-gather input for the sharded engines).
    dstep: optional device fp32 step count (already incremented): the kernel derives the bias corrections
    from it, so the launch replays correctly inside a captured HIP graph (``step`` is then ignored).
    emas / ema_decay: optional fp32 parameter averages (one per parameter, None where a parameter keeps none) updated
    in the same launch from the new fp32 parameter: ``ema += (1 - ema_decay) * (p - ema)``; a skipped step leaves
    them alone.  ``ema_table``: the cached ``PointerTable`` of ``emas`` that goes with ``table``."""
    ema_w = _ema_weight(emas, ema_decay, "adamw_step", len(params))
    if dstep is not None and params and params[0].device.type != "cuda":
        step = int(dstep.item())
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    step_size = lr / bc1
    bc2_sqrt = math.sqrt(bc2)
    if len(params) == 0:
        return
    dev = params[0].device
    if dev.type != "cuda":
        if found_inf is not None and int(found_inf.reshape(-1)[0]) != 0:
            return
        gs = None if grad_scale is None else grad_scale.reshape(())
        for i, p in enumerate(params):
            g = grads[i].float()
            if gs is not None:
                g = g * gs
            m, v = exp_avgs[i], exp_avg_sqs[i]
            if decoupled:
                p.mul_(1 - lr * weight_decay)
            elif weight_decay != 0:
                g = g + weight_decay * p
            m.mul_(beta1).add_(g, alpha=1 - beta1)
            v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
            denom = v.sqrt() / bc2_sqrt + eps
            p.addcdiv_(m, denom, value=-step_size)
            if ema_w is not None and emas[i] is not None:
                _ema_cpu_(emas[i], p, ema_w)
            if out_bf16 is not None and out_bf16[i] is not None:
                out_bf16[i].copy_(p)
        return
    gdt = grads[0].dtype
    if table is None:
        cols = [list(params), list(grads), list(exp_avgs), list(exp_avg_sqs)]
        cols.append(list(out_bf16) if out_bf16 is not None else [None] * len(params))
        table = _cache.get(("adamw", gdt, len(params), id(params[0])), cols)
    if ema_w is not None:
        if ema_table is None:
            ema_table = _cache.get_pointers(("adamw-ema", gdt, len(params), id(params[0])), list(emas), list(params))
        _lib.call("pdt_adamw_ema_mt", table.meta.data_ptr(), table.blk.data_ptr(), table.nblocks, table.chunk,
                  _lib.dtype_code(gdt), float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
                  float(step_size), float(bc2_sqrt), 1 if decoupled else 0, _lib.ptr(grad_scale),
                  _lib.ptr(found_inf), _lib.ptr(dstep), ema_table.ptrs.data_ptr(), ema_w, _lib.stream_handle(dev))
        return
    _lib.call("pdt_adamw_mt", table.meta.data_ptr(), table.blk.data_ptr(), table.nblocks, table.chunk,
              _lib.dtype_code(gdt), float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
              float(step_size), float(bc2_sqrt), 1 if decoupled else 0, _lib.ptr(grad_scale), _lib.ptr(found_inf),
              _lib.ptr(dstep), _lib.stream_handle(dev))


def sgd_step(params, grads, bufs, *, lr, momentum: float, weight_decay: float, nesterov: bool,
             grad_scale: torch.Tensor | None = None, found_inf: torch.Tensor | None = None, out_bf16=None,
             table: TensorTable | None = None, emas=None, ema_decay: float | None = None,
             ema_table: PointerTable | None = None) -> None:
    """One fused (multi-tensor) SGD update, torch.optim.SGD's math with dampening 0 (torch/optim/sgd.py
    ``_single_tensor_sgd``).  fp32 params / momentum buffers; grads fp32 or bf16.

    lr: a float, or a 1-element fp32 tensor on the parameters' device -- the kernel then reads the rate from the
    device, so a launch captured into a HIP graph follows a schedule that ``fill_``s the tensor.
    bufs: the momentum buffers (zeros before the first step); ignored, and may be None, when ``momentum`` is 0.
    grad_scale / found_inf / out_bf16 / table / emas / ema_decay / ema_table: as in ``adamw_step``."""
    ema_w = _ema_weight(emas, ema_decay, "sgd_step", len(params))
    if len(params) == 0:
        return
    dev = params[0].device
    use_mom = momentum != 0
    if use_mom:
        assert bufs is not None and len(bufs) == len(params) and all(b is not None for b in bufs), \
            "sgd_step: momentum != 0 needs a buffer per parameter"
    if dev.type != "cuda":
        if found_inf is not None and int(found_inf.reshape(-1)[0]) != 0:
            return
        gs = None if grad_scale is None else grad_scale.reshape(())
        rate = lr.reshape(()).to(torch.float32) if torch.is_tensor(lr) else float(lr)
        for i, p in enumerate(params):
            g = grads[i].float()
            if gs is not None:
                g = g * gs
            if weight_decay != 0:
                g = g + weight_decay * p
            if use_mom:
                b = bufs[i]
                b.mul_(momentum).add_(g)
                g = g.add(b, alpha=momentum) if nesterov else b
            if torch.is_tensor(rate):
                p.sub_(g * rate)
            else:
                p.add_(g, alpha=-rate)
            if ema_w is not None and emas[i] is not None:
                _ema_cpu_(emas[i], p, ema_w)
            if out_bf16 is not None and out_bf16[i] is not None:
                out_bf16[i].copy_(p)
        return
    gdt = grads[0].dtype
    if gdt not in (torch.float32, torch.bfloat16):
        raise TypeError(f"sgd_step: gradients must be fp32 or bf16, got {gdt}")
    if torch.is_tensor(lr):
        if lr.dtype != torch.float32 or lr.numel() != 1 or lr.device != dev:
            raise TypeError("sgd_step: a tensor lr must be one fp32 element on the parameters' device")
        lr_ptr, lr_val = lr.data_ptr(), 0.0
    else:
        lr_ptr, lr_val = 0, float(lr)
    if table is None:
        none = [None] * len(params)
        cols = [list(params), list(grads), list(bufs) if use_mom else none, none,
                list(out_bf16) if out_bf16 is not None else none]
        table = _cache.get(("sgd", gdt, len(params), id(params[0])), cols)
    if ema_w is not None:
        if ema_table is None:
            ema_table = _cache.get_pointers(("sgd-ema", gdt, len(params), id(params[0])), list(emas), list(params))
        _lib.call("pdt_sgd_ema_mt", table.meta.data_ptr(), table.blk.data_ptr(), table.nblocks, table.chunk,
                  _lib.dtype_code(gdt), lr_val, float(momentum), float(weight_decay), 1 if nesterov else 0,
                  _lib.ptr(grad_scale), _lib.ptr(found_inf), lr_ptr, ema_table.ptrs.data_ptr(), ema_w,
                  _lib.stream_handle(dev))
        return
    _lib.call("pdt_sgd_mt", table.meta.data_ptr(), table.blk.data_ptr(), table.nblocks, table.chunk,
              _lib.dtype_code(gdt), lr_val, float(momentum), float(weight_decay), 1 if nesterov else 0,
              _lib.ptr(grad_scale), _lib.ptr(found_inf), lr_ptr, _lib.stream_handle(dev))


def _lamb_bias(beta1, beta2, step, dstep, params):
    if dstep is not None and params and params[0].device.type != "cuda":
        step = int(dstep.item())
    step = max(int(step), 1)
    return 1.0 - beta1 ** step, math.sqrt(1.0 - beta2 ** step)


def _lamb_u_cpu(p, m, v, bc1, bc2_sqrt, eps, wd):
    """The LAMB update direction from the new moments and the old parameter (the kernels' ``lamb_update``)."""
    return (m / bc1) / (v.sqrt() / bc2_sqrt + eps) + wd * p


def _lamb_tables(name, params, grads, exp_avgs, exp_avg_sqs, out_bf16, gids, table, row_table):
    if table is None:
        cols = [list(params), list(grads), list(exp_avgs), list(exp_avg_sqs),
                list(out_bf16) if out_bf16 is not None else [None] * len(params)]
        table = _cache.get((name, grads[0].dtype, len(params), id(params[0])), cols)
    if row_table is None:
        row_table = _cache.get_rows((name + "-rows", grads[0].dtype, len(params), id(params[0])), table, gids)
    if row_table.nrows != len(params) or list(row_table.gids) != [int(g) for g in gids]:
        raise ValueError("lamb: the row table does not belong to these rows")
    return table, row_table


def lamb_stage1(params, grads, exp_avgs, exp_avg_sqs, sums: torch.Tensor, *, beta1: float, beta2: float, eps: float,
                weight_decay: float, step: int, gids, grad_scale: torch.Tensor | None = None,
                found_inf: torch.Tensor | None = None, out_bf16=None, table: TensorTable | None = None,
                row_table: RowTable | None = None, dstep: torch.Tensor | None = None) -> None:
    """First pass of ``lamb_step`` over one list of rows: the new moments are stored and ``sums[gids[i]]`` receives
    row i's (``sum p*p``, ``sum u*u``) -- one stage-1 launch and one row-sum launch.  ``sums``: the caller's zeroed
    ``[n_logical, 2]`` fp32 tensor (several row lists of one param group share it)."""
    if len(params) == 0:
        return
    if sums.dtype != torch.float32 or sums.dim() != 2 or sums.shape[1] != 2 or not sums.is_contiguous() or \
            sums.device != params[0].device:
        raise TypeError("lamb: sums is a contiguous [n_logical, 2] fp32 tensor on the parameters' device")
    if len(gids) != len(params) or min(gids) < 0 or max(gids) >= sums.shape[0]:
        raise ValueError(f"lamb: one logical-tensor index in [0, {sums.shape[0]}) per row")
    bc1, bc2_sqrt = _lamb_bias(beta1, beta2, step, dstep, params)
    dev = params[0].device
    if dev.type != "cuda":
        if found_inf is not None and int(found_inf.reshape(-1)[0]) != 0:
            return
        gs = None if grad_scale is None else grad_scale.reshape(())
        for i, p in enumerate(params):
            g = grads[i].float()
            if gs is not None:
                g = g * gs
            m, v = exp_avgs[i], exp_avg_sqs[i]
            m.mul_(beta1).add_(g, alpha=1 - beta1)
            v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
            u = _lamb_u_cpu(p, m, v, bc1, bc2_sqrt, eps, weight_decay)
            sums[gids[i], 0] = (p * p).sum()
            sums[gids[i], 1] = (u * u).sum()
        return
    gdt = grads[0].dtype
    if gdt not in (torch.float32, torch.bfloat16):
        raise TypeError(f"lamb: gradients must be fp32 or bf16, got {gdt}")
    table, row_table = _lamb_tables("lamb", params, grads, exp_avgs, exp_avg_sqs, out_bf16, gids, table, row_table)
    partial = torch.empty(2 * max(table.nblocks, 1), dtype=torch.float32, device=dev)
    st = _lib.stream_handle(dev)
    _lib.call("pdt_lamb_stage1_mt", table.meta.data_ptr(), table.blk.data_ptr(), table.nblocks, table.chunk,
              _lib.dtype_code(gdt), float(beta1), float(beta2), 1.0 - float(beta1), 1.0 - float(beta2), float(eps),
              float(weight_decay), float(bc1), float(bc2_sqrt), _lib.ptr(grad_scale), _lib.ptr(found_inf), _lib.ptr(dstep), partial.data_ptr(), st)
    _lib.call("pdt_lamb_rowsum", partial.data_ptr(), row_table.rows.data_ptr(), row_table.nrows, _lib.ptr(found_inf),
              sums.data_ptr(), st)


def lamb_stage2(params, exp_avgs, exp_avg_sqs, sums: torch.Tensor, *, lr: float, beta1: float, beta2: float,
                eps: float, weight_decay: float, step: int, adapt: bool, gids, found_inf: torch.Tensor | None = None,
                out_bf16=None, table: TensorTable | None = None, row_table: RowTable | None = None,
                dstep: torch.Tensor | None = None, emas=None, ema_decay: float | None = None,
                ema_table: PointerTable | None = None) -> None:
    """Second pass of ``lamb_step``: ``p -= lr * r * u`` with ``r`` from ``sums[gids[i]]`` (all-reduced by the caller
    where a logical tensor spans ranks), the bf16 copy and the parameter EMA -- one launch.  ``table`` / ``row_table``
    are stage 1's."""
    ema_w = _ema_weight(emas, ema_decay, "lamb_step", len(params))
    if len(params) == 0:
        return
    bc1, bc2_sqrt = _lamb_bias(beta1, beta2, step, dstep, params)
    dev = params[0].device
    if dev.type != "cuda":
        if found_inf is not None and int(found_inf.reshape(-1)[0]) != 0:
            return
        for i, p in enumerate(params):
            u = _lamb_u_cpu(p, exp_avgs[i], exp_avg_sqs[i], bc1, bc2_sqrt, eps, weight_decay)
            pn, un = sums[gids[i], 0], sums[gids[i], 1]
            if adapt and float(pn) > 0 and float(un) > 0:
                p.sub_(u * (lr * (pn.sqrt() / un.sqrt())))
            else:
                p.sub_(u * lr)
            if ema_w is not None and emas[i] is not None:
                _ema_cpu_(emas[i], p, ema_w)
            if out_bf16 is not None and out_bf16[i] is not None:
                out_bf16[i].copy_(p)
        return
    if table is None or row_table is None:
        raise ValueError("lamb_stage2: pass the table and the row table stage 1 used")
    args = (table.meta.data_ptr(), table.blk.data_ptr(), table.nblocks, table.chunk, float(lr), float(beta1),
            float(beta2), 1.0 - float(beta1), 1.0 - float(beta2), float(eps), float(weight_decay), float(bc1),
            float(bc2_sqrt), 1 if adapt else 0,
            _lib.ptr(found_inf), _lib.ptr(dstep), row_table.rows.data_ptr(), sums.data_ptr())
    if ema_w is not None:
        if ema_table is None:
            ema_table = _cache.get_pointers(("lamb-ema", len(params), id(params[0])), list(emas), list(params))
        _lib.call("pdt_lamb_stage2_ema_mt", *args, ema_table.ptrs.data_ptr(), ema_w, _lib.stream_handle(dev))
        return
    _lib.call("pdt_lamb_stage2_mt", *args, _lib.stream_handle(dev))


def lamb_step(params, grads, exp_avgs, exp_avg_sqs, *, lr: float, beta1: float, beta2: float, eps: float,
              weight_decay: float, step: int, adapt: bool, gids, n_logical: int, sums: torch.Tensor | None = None,
              reduce=None, grad_scale: torch.Tensor | None = None, found_inf: torch.Tensor | None = None,
              out_bf16=None, table: TensorTable | None = None, row_table: RowTable | None = None,
              dstep: torch.Tensor | None = None, emas=None, ema_decay: float | None = None,
              ema_table: PointerTable | None = None) -> torch.Tensor:
    """One fused (multi-tensor) LAMB update.  fp32 params/state; grads fp32 or bf16.  Row i is logical tensor
    ``gids[i]`` of ``n_logical``, or the local part of it:

        g = grad * grad_scale;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g
        u = (m / (1 - b1^t)) / (sqrt(v) / sqrt(1 - b2^t) + eps) + wd p
        r = ||p|| / ||u||  if adapt and both norms > 0, else 1;   p -= lr r u

    with the norms over the whole logical tensor and the parameter before the update.  On CUDA: stage 1 (moments,
    per-block partial sums), the row sum, ``reduce(sums)`` when given (the all-reduce of an engine that cuts tensors
    across ranks), stage 2 -- no host sync.  Returns ``sums``, the ``[n_logical, 2]`` fp32 device tensor of
    (``||p||^2``, ``||u||^2``) (zero-filled here; pass one to reuse its storage).  The other arguments are
    ``adamw_step``'s; ``row_table`` is the cached ``RowTable`` of ``gids`` that goes with ``table``."""
    if len(params) == 0:
        return sums if sums is not None else torch.zeros(int(n_logical), 2, dtype=torch.float32)
    if sums is None:
        sums = torch.zeros(int(n_logical), 2, dtype=torch.float32, device=params[0].device)
    else:
        if sums.shape[0] != int(n_logical):
            raise ValueError(f"lamb_step: sums has {sums.shape[0]} rows for {n_logical} logical tensors")
        sums.zero_()
    gids = [int(g) for g in gids]
    if params[0].device.type == "cuda":
        table, row_table = _lamb_tables("lamb", params, grads, exp_avgs, exp_avg_sqs, out_bf16, gids, table,
                                        row_table)
    lamb_stage1(params, grads, exp_avgs, exp_avg_sqs, sums, beta1=beta1, beta2=beta2, eps=eps,
                weight_decay=weight_decay, step=step, gids=gids, grad_scale=grad_scale, found_inf=found_inf,
                out_bf16=out_bf16, table=table, row_table=row_table, dstep=dstep)
    if reduce is not None:
        reduce(sums)
    lamb_stage2(params, exp_avgs, exp_avg_sqs, sums, lr=lr, beta1=beta1, beta2=beta2, eps=eps,
                weight_decay=weight_decay, step=step, adapt=adapt, gids=gids, found_inf=found_inf, out_bf16=out_bf16,
                table=table, row_table=row_table, dstep=dstep, emas=emas, ema_decay=ema_decay, ema_table=ema_table)
    return sums


def swap_(a_list: Sequence[torch.Tensor], b_list: Sequence[torch.Tensor], out_bf16=None,
          table: TensorTable | None = None) -> None:
    """Exchange two lists of fp32 tensors element by element (``a <-> b``) in ONE launch on CUDA; ``out_bf16[i]``
    (bf16, or None) receives the new ``a`` with the optimizer epilogue's rounding.  A second call undoes the first
    exactly.  Puts parameter averages (``b``) into the fp32 masters (``a``) and refreshes the compute copy."""
    a_list, b_list = list(a_list), list(b_list)
    if len(a_list) != len(b_list):
        raise ValueError("swap_: the two lists differ in length")
    if not a_list:
        return
    outs = list(out_bf16) if out_bf16 is not None else [None] * len(a_list)
    for a, b, o in zip(a_list, b_list, outs):
        if a.dtype != torch.float32 or b.dtype != torch.float32 or a.numel() != b.numel() or a.device != b.device:
            raise TypeError("swap_: pairs of fp32 tensors of equal size on one device")
        if o is not None and (o.dtype != torch.bfloat16 or o.numel() != a.numel() or o.device != a.device):
            raise TypeError("swap_: out_bf16 entries are bf16 tensors of the pair's size and device")
    dev = a_list[0].device
    if dev.type != "cuda":
        for a, b, o in zip(a_list, b_list, outs):
            t = a.clone()
            a.copy_(b)
            b.copy_(t)
            if o is not None:
                o.copy_(a)
        return
    if table is None:
        table = _cache.get(("swap", len(a_list), id(a_list[0])), [a_list, b_list, outs])
    _lib.call("pdt_swap_mt", table.meta.data_ptr(), table.blk.data_ptr(), table.nblocks, table.chunk,
              _lib.stream_handle(dev))


def step_inc_(dstep: torch.Tensor, found_inf: torch.Tensor | None = None) -> None:
    """dstep += 1 unless ``found_inf`` (device int32 flag) is set -- on the device, no host sync."""
    if dstep.device.type != "cuda":
        if found_inf is None or int(found_inf.reshape(-1)[0]) == 0:
            dstep.add_(1.0)
        return
    _lib.call("pdt_step_inc", dstep.data_ptr(), _lib.ptr(found_inf), _lib.stream_handle(dstep.device))


def cast_f32_to_bf16(src: torch.Tensor, dst: torch.Tensor) -> None:
    assert src.dtype == torch.float32 and dst.dtype == torch.bfloat16 and src.numel() == dst.numel()
    if src.device.type != "cuda":
        dst.copy_(src)
        return
    _lib.call("pdt_cast_f32_bf16", src.data_ptr(), dst.data_ptr(), src.numel(), _lib.stream_handle(src.device))


def add_(dsts: Sequence[torch.Tensor], srcs: Sequence[torch.Tensor | None], name: str = "add") -> None:
    """dst += src for every pair (same dtype, same element order; a None src adds nothing) in ONE launch on CUDA
    (bf16 / fp32) -- per-parameter gradients accumulated into a flat buffer."""
    pairs = [(d, s) for d, s in zip(dsts, srcs) if s is not None]
    if not pairs:
        return
    dev = pairs[0][0].device
    if dev.type != "cuda" or pairs[0][0].dtype not in (torch.bfloat16, torch.float32) or \
            torch.cuda.is_current_stream_capturing():
        torch._foreach_add_([d for d, _ in pairs], [s for _, s in pairs])
        return
    for d, s in pairs:
        assert s.dtype == d.dtype and s.numel() == d.numel()
    t = _cache.get(name, [[d for d, _ in pairs], [s for _, s in pairs]])
    _lib.call("pdt_add_mt", t.meta.data_ptr(), t.blk.data_ptr(), t.nblocks, t.chunk, _lib.dtype_code(pairs[0][0].dtype),
              _lib.stream_handle(dev))


def copy_(dsts: Sequence[torch.Tensor], srcs: Sequence[torch.Tensor | None], name: str = "copy") -> None:
    """dst.copy_(src) for every pair (same dtype, same element order; a None src zero-fills its dst) in ONE
    launch on CUDA -- e.g. per-parameter gradients gathered into a flat buffer."""
    if not dsts:
        return
    dev = dsts[0].device
    if dev.type != "cuda":
        for d, s in zip(dsts, srcs):
            d.zero_() if s is None else d.copy_(s)
        return
    for d, s in zip(dsts, srcs):
        assert s is None or (s.dtype == d.dtype and s.numel() == d.numel())
    key = TensorTable.make_key([list(dsts), list(srcs)])
    cached = _cache._tables.get(name)
    if torch.cuda.is_current_stream_capturing() and (cached is None or cached.key() != key):
        # a new pointer set while a HIP graph is captured: no table upload is allowed -- torch's foreach copy
        pairs = [(d, s) for d, s in zip(dsts, srcs) if s is not None]
        if pairs:
            torch._foreach_copy_([d for d, _ in pairs], [s for _, s in pairs])
        zs = [d for d, s in zip(dsts, srcs) if s is None]
        if zs:
            torch._foreach_zero_(zs)
        return
    t = _cache.get(name, [list(dsts), list(srcs)])
    _lib.call("pdt_copy_mt", t.meta.data_ptr(), t.blk.data_ptr(), t.nblocks, t.chunk, dsts[0].element_size(),
              _lib.stream_handle(dev))
