"""Dropout without a stored mask: the keep decision of element ``e`` is a pure function of ``(key, e)``.

The definition (csrc/kernels/philox.h; the kernels, the torch fallback below and tests/dropout_ref.py share it):

* Philox4x32-10 (Random123 constants).  ``key`` is an ``int64[1]`` tensor the kernel reads from device memory --
  never a host scalar, so a captured graph sees the fresh keys of each replay; ``k0`` / ``k1`` are its low / high
  32 bits.
* element ``e`` (row-major linear index of the contiguous tensor, 64-bit): group ``g = e >> 3``, counter
  ``(g & 0xffffffff, g >> 32, 0, 0)``; one call yields ``w0..w3`` for the group's eight elements, and element
  ``j = e & 7`` draws ``u = (w[j >> 1] >> (16 * (j & 1))) & 0xffff``.
* ``thr = min(65535, round(p * 65536))``, keep iff ``u >= thr``, ``scale = 65536 / (65536 - thr)``: ``p`` is
  quantised to 1/65536 and the scale is exactly unbiased for the quantised rate.

Keys come from ``draw_keys`` -- ``random_()`` on the device's torch generator -- so masks follow
``torch.manual_seed`` (each rank's masks follow its own generator), a key handed to a checkpointed block is saved
and not redrawn, and drawing works under graph capture.  bf16 / fp32 GPU tensors run the HIP kernels
(csrc/kernels/dropout.hip); CPU tensors and other dtypes build the IDENTICAL mask with torch ops, which makes a CPU
fp32 model a reference for the GPU bf16 one.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib

_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK32 = 0xFFFFFFFF


def quantise(p: float):
    """``(thr, scale)`` of a drop rate ``0 <= p < 1`` (module docstring)."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout rate must satisfy 0 <= p < 1, got {p}")
    thr = min(65535, int(round(p * 65536)))
    return thr, 65536.0 / (65536 - thr)


def draw_keys(n: int, device) -> torch.Tensor:
    """``int64[n]`` fresh keys from torch's generator of ``device``.  Models call this through the module
    attribute (``dropout.draw_keys``), so a test can patch it."""
    return torch.empty(n, dtype=torch.int64, device=device).random_()


# ---- torch-op fallback: the same Philox in int64 lanes -------------------------------------------------------
def _mulhilo(m: int, c: torch.Tensor):
    """(hi, lo) 32-bit words of m * c for 32-bit values held in int64.  The full product exceeds the int64 sign
    bit, so c is split into 16-bit halves (each partial product is below 2^48)."""
    a = m * (c & 0xFFFF)
    b = m * (c >> 16)
    lo = (a + ((b & 0xFFFF) << 16)) & _MASK32
    hi = ((a >> 16) + b) >> 16
    return hi, lo


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on int64 tensors holding 32-bit words (broadcast against each other); returns four words."""
    for _ in range(10):
        hi0, lo0 = _mulhilo(_M0, c0)
        hi1, lo1 = _mulhilo(_M1, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + _W0) & _MASK32
        k1 = (k1 + _W1) & _MASK32
    return c0, c1, c2, c3


def keep_mask(numel: int, key: torch.Tensor, thr: int, device=None) -> torch.Tensor:
    """bool[numel]: the keep decisions of elements 0..numel-1 under ``key`` (torch ops, any device)."""
    device = key.device if device is None else device
    k = key.reshape(-1)[:1].to(device=device, dtype=torch.int64)
    k0, k1 = k & _MASK32, (k >> 32) & _MASK32
    g = torch.arange((numel + 7) // 8, dtype=torch.int64, device=device)
    zero = torch.zeros_like(g)
    w = torch.stack(philox4x32_10(g & _MASK32, g >> 32, zero, zero, k0, k1), dim=1)        # [groups, 4]
    u = torch.stack((w & 0xFFFF, (w >> 16) & 0xFFFF), dim=2).reshape(-1)                   # j = 2 * word + half
    return u[:numel] >= thr


def _native(x) -> bool:
    return x.is_cuda and x.dtype in (torch.float32, torch.bfloat16)


def _aligned(t):
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _check_key(key, like):
    if key.dtype != torch.int64 or key.numel() != 1 or key.device != like.device:
        raise ValueError("dropout key must be an int64[1] tensor on the input's device")


def _apply(x, key, thr, scale):
    """keep ? x * scale : 0 over the contiguous ``x`` (forward and backward are the same map)."""
    if x.numel() == 0:
        return torch.empty_like(x)
    if _native(x):
        _check_key(key, x)
        x = _aligned(x)
        y = torch.empty_like(x)
        _lib.call("pdt_dropout_fwd", x.data_ptr(), y.data_ptr(), x.numel(), key.data_ptr(), thr, scale,
                  _lib.dtype_code(x.dtype), _lib.stream_handle(x.device))
        return y
    keep = keep_mask(x.numel(), key, thr, x.device).view(x.shape)
    return torch.where(keep, x * scale, torch.zeros((), dtype=x.dtype, device=x.device))


def dropout_bwd(dy2, key, thr, scale, colsum_dtype=None):
    """``(dx, colsum | None)`` for a contiguous ``[rows, N]`` gradient: dx = keep ? dy * scale : 0 and, with
    ``colsum_dtype``, the column sums of dx as stored (fp32 accumulation of the rounded values) from the same
    pass -- the gradient of a bias added in front of the mask."""
    rows, n = dy2.shape
    if colsum_dtype is None or dy2.numel() == 0:
        dx = _apply(dy2, key, thr, scale)
        return dx, (None if colsum_dtype is None else torch.zeros(n, dtype=colsum_dtype, device=dy2.device))
    if not _native(dy2):
        dx = _apply(dy2, key, thr, scale)
        return dx, dx.float().sum(0).to(colsum_dtype)
    if n % 8 != 0 or colsum_dtype not in (torch.float32, torch.bfloat16):
        from .activations import _colsum
        dx = _apply(dy2, key, thr, scale)
        if colsum_dtype in (torch.float32, torch.bfloat16):
            return dx, _colsum(dx, colsum_dtype)
        return dx, _colsum(dx, torch.float32).to(colsum_dtype)
    _check_key(key, dy2)
    lib = _lib.require()
    dy2 = _aligned(dy2)
    dx = torch.empty_like(dy2)
    cs = torch.empty(n, dtype=colsum_dtype, device=dy2.device)
    ws = torch.empty(lib.pdt_dropout_bwd_ws_floats(rows, n), dtype=torch.float32, device=dy2.device)
    _lib.call("pdt_dropout_bwd", dy2.data_ptr(), dx.data_ptr(), dy2.numel(), key.data_ptr(), thr, scale,
              _lib.dtype_code(dy2.dtype), cs.data_ptr(), _lib.dtype_code(colsum_dtype), rows, n, ws.data_ptr(),
              _lib.stream_handle(dy2.device))
    return dx, cs


class _DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, key, thr, scale):
        ctx.save_for_backward(key)
        ctx.thr, ctx.scale = thr, scale
        return _apply(x.contiguous(), key, thr, scale)

    @staticmethod
    def backward(ctx, dy):
        (key,) = ctx.saved_tensors
        return _apply(dy.contiguous(), key, ctx.thr, ctx.scale), None, None, None


def dropout(x, p: float, key: torch.Tensor, training: bool = True):
    """Inverted dropout of ``x`` at rate ``p`` under ``key`` (``int64[1]``, see ``draw_keys``); the backward
    regenerates the mask from the key -- nothing but the key is saved."""
    thr, scale = quantise(p)
    if not training or thr == 0:
        return x
    return _DropoutFn.apply(x, key, thr, scale)


class Dropout(nn.Module):
    """Drop-in for ``torch.nn.Dropout`` (out of place) on the mask-free kernels: a fresh key per call."""

    def __init__(self, p: float = 0.5):
        super().__init__()
        quantise(p)
        self.p = float(p)

    def forward(self, x):
        if not self.training or self.p == 0.0:
            return x
        return dropout(x, self.p, draw_keys(1, x.device), True)

    def extra_repr(self):
        return f"p={self.p}"
