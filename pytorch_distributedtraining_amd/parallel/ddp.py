"""Bucketed data-parallel engine (replaces torch DDP's C++ Reducer on the reference's DDP path).

Reference behaviour reproduced (Stoke-DDP.py:190-193,248 DDPConfig / distributed=ddp; semantics of
torch/nn/parallel/distributed.py:864-870 startup broadcast, :1198-1229 bucket order + first-iteration
rebuild, :1442-1468 no_sync, :1558 buffer broadcast; reducer.hpp:30-31 bucket caps):

MI355X-first design:
  * ONE flat layout for everything: the native ``BucketPlanner`` orders parameters into buckets
    (reverse registration order, first bucket small so communication starts early, later buckets
    large -- 64 MiB default, chosen by arithmetic so a ring step per xGMI link would stay bandwidth- rather
    than latency-bound; a default, unmeasured on a multi-GPU node), and the model parameters, their gradients (``gradient_as_bucket_view``: autograd
    accumulates straight into the bucket, no copy-in) and -- with ``compute_dtype`` -- the fp32 master
    copy all share that layout.  The optimizer then updates the whole model with ONE fused optimizer
    launch reading bf16 grads and writing the bf16 compute params in its epilogue.
  * Readiness is tracked by the native ``ReadyTracker``; buckets are released strictly in order and
    all-reduced (AVG, fused averaging inside RCCL) asynchronously on the RCCL stream while backward
    continues.  The end-of-backward callback makes the compute stream wait -- no host sync.
  * Buffers (BN running stats) are broadcast coalesced (one collective per dtype) each forward.
"""
from __future__ import annotations

import warnings
import weakref
from contextlib import contextmanager

import torch
import torch.nn as nn

from ..utils import profiling as prof
from ..utils.native import require_runtime
from ._readiness import NullReadiness, Readiness
from ._segments import Segments
from .comm import Comm, default_comm

_DT_ID = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2, torch.float64: 3}


def sync_buffers(module: nn.Module, comm: Comm, holder, mode: str = "changed") -> None:
    """Broadcast rank 0's buffers -- only the ones that changed since the last sync.

    torch DDP re-broadcasts every buffer every forward; SwinIR-S carries ~13 MB of constant buffers
    (relative_position_index, shift masks) against 3.6 MB of gradients.  A buffer's autograd version
    counter moves exactly when it is written in place (BatchNorm running stats, num_batches_tracked),
    identically on every rank, so all ranks pick the same set without a collective.  The first sync
    sends everything; running statistics of norm layers (updated inside the batch-norm kernels, no
    version bump) are always sent; ``mode="all"`` restores torch's behaviour.  ``holder`` keeps the
    version snapshot between calls (DDP and ShardedDataParallel both use this)."""
    bufs = list(module.buffers())
    if not bufs:
        return
    seen = getattr(holder, "_buf_versions", None)
    if mode == "all" or seen is None or len(seen) != len(bufs):
        send = bufs
    else:
        stats = _running_stat_ids(module)
        send = [b for b, v in zip(bufs, seen) if b._version != v or id(b) in stats]
    if send:
        comm.broadcast_coalesced(send)
    holder._buf_versions = [b._version for b in bufs]


def _running_stat_ids(module):
    # norm running statistics are updated inside the batch-norm kernels without a version bump:
    # always treat them as mutable
    ids = set()
    for mod in module.modules():
        for name in ("running_mean", "running_var", "num_batches_tracked"):
            b = getattr(mod, name, None)
            if isinstance(b, torch.Tensor):
                ids.add(id(b))
    return ids


def _dense_stride(p):
    """p's strides when p is dense (contiguous or channels_last: its numel elements fill one span), else the
    contiguous strides of its shape."""
    if p.is_contiguous() or (p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last)):
        return p.stride()
    return torch.empty(p.shape, device="meta").stride()


def _pview(flat, p, o):
    """Parameter ``p``'s region of a flat buffer at offset ``o``, with p's own (dense) strides: a channels_last conv
    weight keeps channels_last memory order in the flat, so MIOpen takes it as is, no per-call layout change."""
    return torch.as_strided(flat, p.shape, _dense_stride(p), o)


class _FlatGroup:
    """All parameters of one storage dtype, laid out bucket after bucket."""

    def __init__(self, params, idxs, buckets, dtype, device, master: bool):
        self.params, self.idxs, self.dtype, self.device = params, idxs, dtype, device
        self.buckets = buckets            # list of (global bucket id, [param local idx], [offsets], numel)
        total = sum(b[3] for b in buckets)
        self.total = total
        self.offset_of = {}
        base = 0
        for (_bid, pl, offs, n) in buckets:
            for li, o in zip(pl, offs):
                self.offset_of[li] = base + o
            base += n
        self.flat_grad = torch.zeros(total, dtype=dtype, device=device)
        self.bucket_views = []
        base = 0
        for (_bid, _pl, _offs, n) in buckets:
            self.bucket_views.append(self.flat_grad[base:base + n])
            base += n
        self.master = None
        self.flat_param = None
        if master:
            # compute-dtype mode: params become views of one flat low-precision buffer that the fused
            # optimizer rewrites from the fp32 master in its epilogue
            self.flat_param = torch.zeros(total, dtype=dtype, device=device)
            with torch.no_grad():
                for li, p in enumerate(params):
                    _pview(self.flat_param, p, self.offset_of[li]).copy_(p.detach())
            for li, p in enumerate(params):
                p.data = _pview(self.flat_param, p, self.offset_of[li])
            m = nn.Parameter(self.flat_param.detach().to(torch.float32))
            m._pdt_lp_shard = self.flat_param
            m._pdt_lp_version = m._version
            m._pdt_grad = self.flat_grad
            m._pdt_zero_grad = self.flat_grad.zero_   # optimizer.zero_grad() clears the accumulated flat grad
            self.master = m
            self.set_segments()

    def set_segments(self):
        """Tell per-tensor optimizers (FusedLAMB) where the parameters lie in the flat master (parallel/_segments.py):
        one span per parameter at its offset, every one whole on this rank (the gradients are all-reduced).  Bucket
        alignment padding belongs to no span."""
        self.master._pdt_segments = Segments([(self.offset_of[li], p.numel(), li) for li, p in enumerate(self.params)],
                                             len(self.params), None)

    def gather_grads(self):
        """Single-process gradient stealing (DistributedDataParallel._steal_grads) with a compute copy: the
        parameters' own (stolen) gradients are ADDED to the flat the fp32 master reads, in ONE multi-tensor launch,
        and then dropped, so the next backward (an accumulation micro-step) steals fresh gradients again instead of
        autograd adding into every parameter's .grad with one kernel each (227 launches per SwinIR-S step).  The flat
        is zeroed by zero_grad / drop_grads, so it holds the accumulated gradient.  Under HIP-graph capture the
        gradients stay attached (their addresses are part of the graph)."""
        from ..ops import multi_tensor as mt
        dsts = [_pview(self.flat_grad, p, self.offset_of[li]) for li, p in enumerate(self.params)]
        srcs = [p.grad for p in self.params]
        same = [s is None or all(a == b for a, b, n in zip(s.stride(), d.stride(), d.shape) if n != 1)
                for s, d in zip(srcs, dsts)]
        if all(same):
            mt.add_(dsts, srcs, name=("ddp_gather", id(self)))
        else:
            for s_, d in zip(srcs, dsts):
                if s_ is not None:
                    d.add_(s_)
        if not (self.flat_grad.is_cuda and torch.cuda.is_current_stream_capturing()):
            for p in self.params:
                p.grad = None

    def drop_grads(self, set_to_none: bool = True):
        """zero_grad for a stealing compute-copy group: set_to_none -> the next backward's gradients are stolen
        again; otherwise they are zeroed in place (addresses kept: HIP-graph replay)."""
        if set_to_none:
            for p in self.params:
                p.grad = None
        else:
            gs = [p.grad for p in self.params if p.grad is not None]
            if gs:
                torch._foreach_zero_(gs)
        self.flat_grad.zero_()
    drop_grads._pdt_set_to_none = True

    def attach_grads(self):
        for li, p in enumerate(self.params):
            o = self.offset_of[li]
            # same strides as the parameter (channels_last convs): autograd accumulates in place
            p.grad = _pview(self.flat_grad, p, o)
            p._pdt_grad_flat = self.flat_grad   # FusedOptimizer.zero_grad zeroes the flat once, views stay attached
            p._pdt_grad_members = self.params   # ... when one optimizer owns every parameter viewing it


def _cast_except_batchnorm(module: nn.Module, dtype: torch.dtype) -> None:
    """``module.to(dtype)`` for every floating parameter / buffer except those owned by batch norms."""
    for m in module.modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            continue
        for p in m.parameters(recurse=False):
            if p.is_floating_point() and p.dtype != dtype:
                p.data = p.data.to(dtype)
        for name, b in list(m.named_buffers(recurse=False)):
            if b is not None and b.is_floating_point() and b.dtype != dtype:
                m._buffers[name] = b.to(dtype)


class DistributedDataParallel(nn.Module):
    """Data parallel wrapper.

    Args:
        module: the model (its parameters are re-pointed into flat buffers on ``device``).
        comm: collective layer (default process group).
        bucket_cap_mb / first_bucket_mb: bucket sizes (defaults 64 / 8 MiB, picked from xGMI link arithmetic and
            unmeasured on a multi-GPU node; torch uses 25 / 1).
        broadcast_buffers: broadcast buffers from rank 0 every forward.
        buffer_sync: "changed" (default) sends only buffers written since the last sync; "all" sends every
            buffer every forward like torch DDP.
        find_unused_parameters: allow parameters that receive no gradient (flushed as zeros).
        compute_dtype: e.g. torch.bfloat16 -> the module runs in bf16, gradients are bf16 and
            all-reduced in bf16, and ``optimizer_parameters()`` returns the fp32 master flat(s)
            (the optimizer writes the bf16 compute copy back); batch-norm layers stay fp32.  None -> classic
            fp32 params + autocast.
        reduce_dtype: optional dtype for the all-reduce payload (bf16 compression of fp32 grads).
        rebuild_buckets: after the first backward, re-plan buckets in the observed gradient order.
    """

    def __init__(self, module: nn.Module, comm: Comm | None = None, device=None, bucket_cap_mb: float = 64.0,
                 first_bucket_mb: float = 8.0, broadcast_buffers: bool = True, find_unused_parameters: bool = False,
                 buffer_sync: str = "changed",
                 compute_dtype: torch.dtype | None = None, reduce_dtype: torch.dtype | None = None,
                 rebuild_buckets: bool = True, device_ids=None, **_ignored):
        super().__init__()
        self.module = module
        self.comm = comm or default_comm()
        if device is None:
            if device_ids:
                device = torch.device("cuda", device_ids[0])
            else:
                try:
                    device = next(module.parameters()).device
                except StopIteration:
                    device = torch.device("cpu")
        self.device = torch.device(device)
        self.broadcast_buffers = broadcast_buffers
        self.buffer_sync = buffer_sync
        self.find_unused_parameters = find_unused_parameters
        self.compute_dtype = compute_dtype
        self.reduce_dtype = reduce_dtype
        self.bucket_cap = int(bucket_cap_mb * (1 << 20))
        self.first_bucket = int(first_bucket_mb * (1 << 20))
        self._rebuild_pending = rebuild_buckets
        self._no_sync = False
        self._handles = []
        self._callback_queued = False
        self._observed = []
        self._warned_unused = False
        self._ready = None
        self._graph_safe = False

        module.to(self.device)
        if compute_dtype is not None:
            # batch norms keep fp32 affine parameters and running statistics (their own fp32 flat group):
            # bf16 running stats drift, and the fused BN kernels take fp32 parameters with bf16 activations.
            # They are never cast at all (a round trip through bf16 would round values loaded before wrapping).
            _cast_except_batchnorm(module, compute_dtype)
        self.params = [p for p in module.parameters() if p.requires_grad]
        # one process: no collective reads the buckets, so the gradients stay where autograd puts them --
        # AccumulateGrad STEALS each freshly produced gradient (no kernel) instead of adding it into a zeroed
        # bucket view (one add launch per parameter per step: 161 for ResNet-50, ~0.7 ms).  With a compute copy
        # the fp32 masters read the flat: one multi-tensor gather fills it at the end of each backward.
        self._steal_grads = self.comm.world_size == 1
        self._gather_queued = False
        if self.comm.world_size > 1:
            self.comm.broadcast_coalesced([p.data for p in self.params] + [b for b in module.buffers()])
        self._build(order=None)

    # ------------------------------------------------------------------ layout
    def _build(self, order):
        rt = require_runtime()
        numels = [p.numel() for p in self.params]
        esz = [p.element_size() if self.reduce_dtype is None else torch.tensor([], dtype=self.reduce_dtype)
               .element_size() for p in self.params]
        dts = [_DT_ID.get(p.dtype, 9) for p in self.params]
        planner = rt.BucketPlanner(numels, esz, dts, self.first_bucket, self.bucket_cap, 16)
        plan = planner.plan(order) if order is not None else planner.plan_default()
        self.plan = plan
        # group buckets by dtype
        groups = {}
        for bid, b in enumerate(plan):
            dt = self.params[b.params[0]].dtype
            groups.setdefault(dt, []).append(bid)
        self.groups = []
        self.bucket_loc = {}       # bucket id -> (group, view index)
        self.param_group = {}      # global param idx -> (group, local idx)
        for dt, bids in groups.items():
            gidx = sorted({i for bid in bids for i in plan[bid].params})
            local = {g: li for li, g in enumerate(gidx)}
            bl = [(bid, [local[i] for i in plan[bid].params], list(plan[bid].offsets), plan[bid].numel)
                  for bid in bids]
            g = _FlatGroup([self.params[i] for i in gidx], gidx, bl, dt, self.device,
                           master=self.compute_dtype is not None)
            for vi, bid in enumerate(bids):
                self.bucket_loc[bid] = (g, vi)
            for li, gi in enumerate(gidx):
                self.param_group[gi] = (g, li)
            self.groups.append(g)
        if not self._steal_grads:
            for g in self.groups:
                g.attach_grads()
        elif self.compute_dtype is not None:
            for g in self.groups:
                if g.master is not None:
                    g.master._pdt_zero_grad = g.drop_grads      # bound method: _pdt_set_to_none via __func__
        self._arm_readiness()

    def _arm_readiness(self):
        """Bucket readiness for the current plan: C++ AccumulateGrad post hooks (one Python call per ready
        bucket) once the plan is final; per-parameter Python hooks while the first iteration records the
        gradient order for the rebuild.  Callbacks hold the engine weakly (the C++ side is invisible to GC)."""
        if self._ready is not None:
            self._ready.remove()
        if self.comm.world_size == 1:
            self._ready = NullReadiness()
            self._rebuild_pending = False       # bucket order only matters to the collectives
            return
        ref = weakref.ref(self)
        self._ready = Readiness(
            self.params, [list(b.params) for b in self.plan],
            on_first=lambda: ref()._queue_finalize(), on_ready=lambda b: ref()._launch(b),
            observe=(lambda i: ref()._observed.append(i)) if self._rebuild_pending else None,
            native=not self._graph_safe)
        self._ready.set_enabled(not self._no_sync)

    def prepare_capture(self):
        """Switch bucket readiness to per-parameter Python hooks before a HIP-graph capture (Trainer.graph at
        world > 1).  The native hooks hold the parameters' AccumulateGrad nodes, which remember the stream
        they were created on (see _readiness.NullReadiness); Python post-accumulate hooks hold no node.  The
        hooks run once, while the step is captured, and the bucket all-reduces they launch (RCCL: the mesh
        is bypassed under capture, parallel/comm.py) are recorded into the graph with the backward."""
        if not self._graph_safe:
            self._graph_safe = True
            if getattr(self._ready, "kind", "none") == "native":
                self._arm_readiness()

    def _rebuild(self):
        """Re-plan buckets in the observed gradient-ready order (first iteration), keeping values."""
        order = list(self._observed)
        seen = set(order)
        order += [i for i in reversed(range(len(self.params))) if i not in seen]
        if order == list(reversed(range(len(self.params)))):
            return
        if any(getattr(g.master, "_pdt_opt_state", False) for g in self.groups):
            # the optimizer already holds moments in the current master layout (e.g. restored from a
            # checkpoint before the first step): a new element order would misalign them -- keep the layout
            warnings.warn("DDP: optimizer state already attached to the flat masters; skipping the bucket rebuild")
            return
        old_master = {id(g): g.master for g in self.groups}
        grads = [p.grad.detach().clone() if p.grad is not None else None for p in self.params]
        masters = {}
        for g in self.groups:
            if g.master is not None:
                for li, gi in enumerate(g.idxs):
                    o = g.offset_of[li]
                    masters[gi] = g.master.detach()[o:o + self.params[gi].numel()].clone()
        self._build(order)
        for i, p in enumerate(self.params):
            if grads[i] is not None:
                p.grad.copy_(grads[i])
        # keep the user-visible master Parameter objects (optimizer may already hold them)
        old = [m for m in old_master.values() if m is not None]
        for g, om in zip(self.groups, old + [None] * len(self.groups)):
            if g.master is None:
                continue
            new = g.master.detach()
            for li, gi in enumerate(g.idxs):
                o = g.offset_of[li]
                new[o:o + self.params[gi].numel()].copy_(masters[gi])
            if om is not None:
                om.data = new
                om._pdt_lp_shard = g.flat_param
                om._pdt_grad = g.flat_grad
                om._pdt_zero_grad = g.flat_grad.zero_
                om._pdt_lp_version = om._version
                g.master = om
                g.set_segments()

    # ------------------------------------------------------------------ hooks (parallel/_readiness.py)
    def _launch(self, bid):
        g, vi = self.bucket_loc[bid]
        view = g.bucket_views[vi]
        if self.comm.world_size == 1:
            return
        with prof.range(f"ddp.all_reduce[bucket {bid}]"):
            self._launch_bucket(view)

    def _launch_bucket(self, view):
        if self.reduce_dtype is not None and self.reduce_dtype != view.dtype:
            payload = view.to(self.reduce_dtype)
            h = self.comm.all_reduce(payload, "avg", async_op=True)
            self._handles.append((h, view, payload))
        else:
            h = self.comm.all_reduce(view, "avg", async_op=True)
            self._handles.append((h, None, None))

    def _queue_finalize(self):
        if self._callback_queued:
            return
        self._callback_queued = True
        torch.autograd.Variable._execution_engine.queue_callback(self._finalize)

    def _finalize(self):
        self._callback_queued = False
        self.comm.check_errors()
        if not self._ready.all_released():
            if not self.find_unused_parameters and not self._warned_unused:
                warnings.warn("DDP: some parameters received no gradient this iteration; their buckets were "
                              "reduced as zeros (pass find_unused_parameters=True to silence)")
                self._warned_unused = True
            for bid in self._ready.flush():
                self._launch(bid)
        for h, view, payload in self._handles:
            h.wait()
            if view is not None:
                view.copy_(payload)
        self._handles.clear()
        self._ready.reset()
        if self._rebuild_pending:
            self._rebuild_pending = False
            self._rebuild()
            self._observed = []
            if self._ready.observing:
                self._arm_readiness()      # order recorded (the plan kept): stop recording, native hooks now

    # ------------------------------------------------------------------ forward
    def forward(self, *args, **kwargs):
        if self.params and self.params[0].grad is None and not self._steal_grads:
            # zero_grad(set_to_none=True) dropped the bucket views: zero the flats and re-attach
            for g in self.groups:
                g.flat_grad.zero_()
                g.attach_grads()
        if self.broadcast_buffers and self.comm.world_size > 1 and self.module.training:
            self._sync_buffers()
        out = self.module(*args, **kwargs)
        if self._steal_grads and self.compute_dtype is not None and torch.is_grad_enabled():
            self._arm_gather(out)
        return out

    def _arm_gather(self, out):
        """Queue the compute-copy gradient gather to run once the backward through ``out`` has finished."""
        from torch.utils._pytree import tree_leaves
        leaves = [out] if torch.is_tensor(out) else tree_leaves(out)
        if not any(torch.is_tensor(t) for t in leaves) and hasattr(out, "__dict__"):
            leaves = tree_leaves(vars(out))          # dataclass / plain object outputs: walk their fields
        for t in leaves:
            if torch.is_tensor(t) and t.requires_grad:
                ref = weakref.ref(self)
                t.register_hook(lambda g, ref=ref: ref()._queue_gather() or g)
                return
        # nothing to hook: if a backward still runs (through a tensor this walk could not see) the masters would
        # step on zero gradients -- say so once instead of failing silently
        if self.module.training and not getattr(self, "_warned_no_hook", False):
            self._warned_no_hook = True
            warnings.warn("DistributedDataParallel(compute_dtype=...): no grad-requiring tensor found in the model "
                          f"output ({type(out).__name__}); the master-gradient gather is not queued for this forward",
                          stacklevel=3)

    def _queue_gather(self):
        if not self._gather_queued:
            self._gather_queued = True
            torch.autograd.Variable._execution_engine.queue_callback(self._gather)

    def _gather(self):
        self._gather_queued = False
        for g in self.groups:
            if g.master is not None:
                g.gather_grads()

    def _sync_buffers(self):
        sync_buffers(self.module, self.comm, self, self.buffer_sync)

    @contextmanager
    def no_sync(self):
        old = self._no_sync
        self._no_sync = True
        self._ready.set_enabled(False)
        try:
            yield
        finally:
            self._no_sync = old
            self._ready.set_enabled(not old)

    # ------------------------------------------------------------------ optimizer / checkpoint helpers
    def optimizer_parameters(self):
        """What the optimizer should step: fp32 masters (compute_dtype mode) or the module params."""
        if self.compute_dtype is not None:
            return [g.master for g in self.groups]
        return list(self.params)

    def parameters_for_clipping(self):
        return self.optimizer_parameters()

    def zero_grad(self, set_to_none: bool = False):
        if self._steal_grads and self.compute_dtype is not None:
            for g in self.groups:
                g.drop_grads(set_to_none)
            return
        if self._steal_grads:
            for p in self.params:
                if set_to_none:
                    p.grad = None
                elif p.grad is not None:
                    p.grad.zero_()
            return
        for g in self.groups:
            g.flat_grad.zero_()

    def full_state_dict(self):
        """Module state dict with fp32 master values for parameters (no 'module.' prefix)."""
        sd = self.module.state_dict()
        if self.compute_dtype is None:
            return sd
        name_of = {id(p): n for n, p in self.module.named_parameters()}
        for g in self.groups:
            for li, gi in enumerate(g.idxs):
                p = self.params[gi]
                sd[name_of[id(p)]] = _pview(g.master.detach(), p, g.offset_of[li]).clone()
        return sd

    def full_optim_state_dict(self, optimizer):
        """compute_dtype mode: the optimizer steps flat fp32 masters; return its state in torch's
        per-parameter layout ({state: {param_idx: {step, exp_avg, exp_avg_sq}}, param_groups}) keyed by the
        module's parameter order, so checkpoints match a plain torch.optim.AdamW over ``module``."""
        if self.compute_dtype is None:
            return optimizer.state_dict()
        idx_of = {id(p): i for i, p in enumerate(self.module.parameters())}
        state = {}
        for g in self.groups:
            st = optimizer.state.get(g.master)
            if not st:
                continue
            for li, gi in enumerate(g.idxs):
                p = self.params[gi]
                o = g.offset_of[li]
                ent = {}
                for k, v in st.items():
                    if torch.is_tensor(v) and v.dim() == 1 and v.numel() == g.master.numel():
                        ent[k] = _pview(v.detach(), p, o).clone()
                    else:
                        ent[k] = v.detach().clone() if torch.is_tensor(v) else v
                state[idx_of[id(p)]] = ent
        groups = []
        for pg in optimizer.param_groups:
            d = {k: v for k, v in pg.items() if k != "params"}
            d["params"] = sorted(idx_of[id(self.params[gi])] for g in self.groups if any(m is g.master for m in
                                                                                        pg["params"])
                                 for gi in g.idxs)
            groups.append(d)
        return {"state": state, "param_groups": groups}

    def load_full_optim_state_dict(self, optimizer, sd):
        if self.compute_dtype is None:
            optimizer.load_state_dict(sd)
            return
        idx_of = {id(p): i for i, p in enumerate(self.module.parameters())}
        if sd.get("param_groups"):
            hp = {k: v for k, v in sd["param_groups"][0].items() if k != "params"}
            for pg in optimizer.param_groups:
                pg.update(hp)
        st_all = sd["state"]
        for g in self.groups:
            new, step = {}, None
            for li, gi in enumerate(g.idxs):
                p = self.params[gi]
                e = st_all.get(idx_of[id(p)], st_all.get(str(idx_of[id(p)])))
                if e is None:
                    continue
                o = g.offset_of[li]
                for k, v in e.items():
                    if torch.is_tensor(v) and v.dim() > 0:
                        if k not in new:
                            new[k] = torch.zeros_like(g.master, dtype=torch.float32)
                        _pview(new[k], p, o).copy_(v.reshape(p.shape))
                    elif k == "step":
                        step = v
            if new:
                if step is not None:
                    new["step"] = step.clone() if torch.is_tensor(step) else torch.tensor(float(step))
                optimizer.state[g.master] = new
                g.master._pdt_opt_state = True
        if hasattr(optimizer, "_dsteps"):
            optimizer._dsteps.clear()

    def load_full_state_dict(self, sd, strict=True):
        res = self.module.load_state_dict(sd, strict=strict)
        if self.compute_dtype is not None:
            name_of = {id(p): n for n, p in self.module.named_parameters()}
            with torch.no_grad():
                for g in self.groups:
                    for li, gi in enumerate(g.idxs):
                        p = self.params[gi]
                        _pview(g.master, p, g.offset_of[li]).copy_(sd[name_of[id(p)]].float())
                    g.master._pdt_lp_version = g.master._version
        return res
