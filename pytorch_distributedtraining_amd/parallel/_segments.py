"""The segment protocol: how an engine tells a per-tensor optimizer (FusedLAMB) where the logical tensors lie inside a
flat optimizer parameter.

An optimizer parameter may carry ``_pdt_segments``, a ``Segments``:

* ``spans``: ``[(start, numel, gid)]`` in the parameter's own flat coordinates -- the local elements of logical tensor
  ``gid``.  Spans do not overlap; elements between them (alignment padding) belong to no tensor.
* ``n_logical``: the number of logical tensors the parameter's ``gid`` s index (those with no local element included).
* ``comm``: None when every logical tensor is whole on this rank; else the ``Comm`` over which per-tensor sums are
  all-reduced (a tensor may be cut by a rank boundary).

DDP sets it on the flat fp32 master of a compute-copy group, FSDP on every unit's flat shard.  OSS partitions whole
parameters and sets nothing.  Optimizers that do not work per tensor (FusedAdamW, FusedSGD) never read it.
"""
from __future__ import annotations

from typing import List, Optional, Tuple


class Segments:
    __slots__ = ("spans", "n_logical", "comm")

    def __init__(self, spans: List[Tuple[int, int, int]], n_logical: int, comm: Optional[object] = None):
        self.spans = [(int(s), int(n), int(g)) for s, n, g in spans]
        self.n_logical = int(n_logical)
        self.comm = comm
        end = 0
        for s, n, g in sorted(self.spans):
            if s < end or n <= 0 or not 0 <= g < self.n_logical:
                raise ValueError(f"Segments: span {(s, n, g)} overlaps its predecessor, is empty or names a tensor "
                                 f"outside [0, {self.n_logical})")
            end = s + n
        if len({g for _, _, g in self.spans}) != len(self.spans):
            raise ValueError("Segments: a logical tensor has one span per parameter")

    def __repr__(self):
        return f"Segments({len(self.spans)} spans of {self.n_logical} tensors, comm={'set' if self.comm else None})"
