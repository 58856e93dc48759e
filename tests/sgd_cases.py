"""The tensor list the fused SGD tests share: the smallest shapes that reach every path of the multi-tensor kernel at
chunk 32768, 256 threads x 4 elements."""
import torch
import torch.nn as nn


def tensor_list(device="cpu", seed=0):
    """Fewer elements than one vector; body + a tail of less than 4; odd 2-D; three chunks, the last with 3
    elements; a 1-D view at storage offset 1 element (misaligned: the scalar path)."""
    g = torch.Generator().manual_seed(seed)
    ts = [torch.randn(s, generator=g) for s in [(5,), (1000,), (33, 17), (65539,)]]
    ts.append(torch.randn(1026, generator=g))
    ts = [t.to(device) for t in ts]
    ts[-1] = ts[-1][1:1025]
    return ts


def clones(ts, dtype=None, param=True):
    """Independent copies with the storage offsets of ``ts`` (a plain clone would realign the view)."""
    out = []
    for t in ts:
        o = t.storage_offset()
        base = torch.empty(o + t.numel() + (1 if o else 0), dtype=dtype or t.dtype, device=t.device)
        v = base[o:o + t.numel()].view(t.shape)
        v.copy_(t)
        out.append(nn.Parameter(v) if param else v)
    return out
