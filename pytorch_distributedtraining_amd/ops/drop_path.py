"""Stochastic depth (drop path): a residual branch is kept or dropped per sample, with no stored mask.

The definition is dropout's (ops/dropout.py, csrc/kernels/philox.h) at per-sample granularity: sample ``b`` of a
site with key ``key`` is kept iff ``dropout.keep_mask(B, key, thr)[b]`` -- the element definition with element index
= sample index -- with ``(thr, scale) = dropout.quantise(rate)``.  tests/dropout_ref.py is therefore its independent
reference as it stands.

The kernels consume per-sample SCALES, not keys: ``sample_scales`` turns the keys of all sites of a forward into one
fp32 ``[sites, B]`` tensor of ``0 | scale`` in one launch (it reads the keys from device memory, so a replayed graph
sees fresh ones), and every consumer -- the scaled window norm (ops.norms), the scaled fused MLP (ops.swin_mlp), the
standalone kernel below -- takes one row of it.  A kept branch is multiplied by its scale; a dropped branch is
selected away, never multiplied by 0: the residual stream's bits pass untouched and a NaN / inf in a dropped branch
reaches neither the output nor any gradient.

``drop_path`` / ``drop_path_add`` run ``csrc/kernels/drop_path.hip`` for bf16 / fp32 GPU tensors; CPU tensors and
other dtypes compute the same map with torch ops (``torch.where``).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib
from . import dropout as _dropout


def site_table(rates, device=None) -> torch.Tensor:
    """fp32 ``[2, sites]``: row 0 the thresholds, row 1 the scales of ``dropout.quantise(rate)`` per site (thr is an
    integer below 2^16, exact in fp32).  Built once per model and device."""
    q = [_dropout.quantise(r) for r in rates]
    return torch.tensor([[float(t) for t, _ in q], [s for _, s in q]], dtype=torch.float32, device=device)


def sample_scales(keys: torch.Tensor, thr_scale: torch.Tensor, batch: int) -> torch.Tensor:
    """fp32 ``[sites, batch]``: ``scale`` where sample b of the site is kept, 0 where it is dropped.  ``keys``
    int64 ``[sites]`` (``dropout.draw_keys``), ``thr_scale`` from ``site_table``.  A site of rate 0 is all ones."""
    sites = keys.numel()
    if keys.dtype != torch.int64 or tuple(thr_scale.shape) != (2, sites) or thr_scale.dtype != torch.float32:
        raise ValueError("sample_scales: keys must be int64[sites] and thr_scale fp32[2, sites]")
    if thr_scale.device != keys.device:
        raise ValueError("sample_scales: keys and thr_scale must be on one device")
    out = torch.empty(sites, batch, dtype=torch.float32, device=keys.device)
    if sites == 0 or batch == 0:
        return out
    if keys.is_cuda:
        keys, thr_scale = keys.contiguous(), thr_scale.contiguous()
        _lib.call("pdt_drop_path_scales", keys.data_ptr(), thr_scale.data_ptr(), out.data_ptr(), sites, batch,
                  _lib.stream_handle(keys.device))
        return out
    zero = torch.zeros((), dtype=torch.float32, device=keys.device)
    for s in range(sites):
        keep = _dropout.keep_mask(batch, keys[s:s + 1], int(thr_scale[0, s].item()))
        out[s] = torch.where(keep, thr_scale[1, s], zero)
    return out


def _native(x) -> bool:
    return x.is_cuda and x.dtype in (torch.float32, torch.bfloat16)


def _aligned(t):
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _check_scale(x, sc):
    if sc.dtype != torch.float32 or sc.dim() != 1 or sc.device != x.device or sc.numel() == 0 \
            or x.numel() % sc.numel() != 0:
        raise ValueError("sample_scale must be an fp32 [B] tensor on the input's device, B dividing the input's size")


def _row_scale(x, res, sc):
    """(res | 0) + (sc[b] != 0 ? x * sc[b] : 0) over the contiguous ``x`` whose B = sc.numel() samples are equal
    contiguous parts (forward and backward are this one map)."""
    _check_scale(x, sc)
    if x.numel() == 0:
        return torch.empty_like(x)
    if _native(x):
        x = _aligned(x)
        res = None if res is None else _aligned(res)
        sc = sc.contiguous()
        y = torch.empty_like(x)
        _lib.call("pdt_drop_path_rows", x.data_ptr(), _lib.ptr(res), y.data_ptr(), x.numel(),
                  x.numel() // sc.numel(), sc.data_ptr(), _lib.dtype_code(x.dtype), _lib.stream_handle(x.device))
        return y
    B = sc.numel()
    xf = x.reshape(B, -1)
    cdt = torch.float32 if x.dtype in (torch.bfloat16, torch.float16) else x.dtype
    s = sc.view(B, 1)
    branch = torch.where(s != 0, xf.to(cdt) * s.to(cdt), torch.zeros((), dtype=cdt, device=x.device))
    if res is not None:
        branch = res.reshape(B, -1).to(cdt) + branch
    return branch.to(x.dtype).view(x.shape)


class _DropPathFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, sc):
        ctx.save_for_backward(sc)
        return _row_scale(x.contiguous(), None, sc)

    @staticmethod
    def backward(ctx, dy):
        (sc,) = ctx.saved_tensors
        return _row_scale(dy.contiguous(), None, sc), None


class _DropPathAddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, r, sc):
        ctx.save_for_backward(sc)
        return _row_scale(r.contiguous(), x.contiguous(), sc)

    @staticmethod
    def backward(ctx, dy):
        (sc,) = ctx.saved_tensors
        return dy, _row_scale(dy.contiguous(), None, sc), None


def drop_path(x, sample_scale):
    """``x`` with sample b multiplied by ``sample_scale[b]``, or exactly 0 where that is 0.  The samples are the
    ``sample_scale.numel()`` equal contiguous parts of ``x`` (its leading dimension, or windows grouped by sample)."""
    return _DropPathFn.apply(x, sample_scale)


def drop_path_add(x, r, sample_scale):
    """``x + drop_path(r)`` in one pass; a dropped sample's rows are ``x`` bit for bit."""
    if r.shape != x.shape and r.numel() != x.numel():
        raise ValueError("drop_path_add: x and r must have one size")
    if r.dtype != x.dtype:
        return x + drop_path(r, sample_scale)
    return _DropPathAddFn.apply(x, r.reshape(x.shape), sample_scale)


class DropPath(nn.Module):
    """Drop-in for timm's ``DropPath`` (per-sample stochastic depth of a residual branch, kept samples scaled by
    1 / keep probability) on the mask-free kernels: a fresh key per call."""

    def __init__(self, drop_prob: float = 0.0):
        super().__init__()
        _dropout.quantise(drop_prob)
        self.drop_prob = float(drop_prob)

    def _table(self, device):
        cache = self.__dict__.setdefault("_table_cache", {})
        t = cache.get(device)
        if t is None:
            t = cache[device] = site_table([self.drop_prob], device)
        return t

    def forward(self, x):
        if not self.training or self.drop_prob == 0.0 or x.numel() == 0:
            return x
        keys = _dropout.draw_keys(1, x.device)
        return drop_path(x, sample_scales(keys, self._table(x.device), x.shape[0])[0])

    def extra_repr(self):
        return f"drop_prob={self.drop_prob}"
