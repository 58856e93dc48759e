#!/usr/bin/env python
"""The fused AdamW and SGD multi-tensor kernels in one process, alternating, 50 launches per timing (bf16 gradient,
bf16 copy-out, as ``bench_kernels.py adamw`` / ``sgd``).  One JSON line per case and round.

Default: several flat sizes, each tensor an allocation of its own -- what a flat's size does to both kernels.
``--offsets``: one size (the first of ``--sizes``), each tensor carved out of its own oversized allocation, tensor
i at element offset ``i * offset`` (multiples of 4 keep the vector path) -- what the relative placement of the
streams does to both kernels at a fixed size."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from bench_kernels import timeit  # noqa: E402

PAD = 8 << 20


def measure(tag, n, rounds, offset=None):
    from pytorch_distributedtraining_amd.ops import adamw_step, sgd_step
    dts = (torch.float32, torch.float32, torch.float32, torch.bfloat16, torch.bfloat16)
    bases = [torch.zeros(n + (0 if offset is None else PAD), device="cuda", dtype=dt) for dt in dts]
    p, m, v, g, lp = (b[i * (offset or 0):i * (offset or 0) + n] for i, b in enumerate(bases))
    p.normal_(), m.normal_(), v.normal_().abs_(), g.normal_()
    for rnd in range(rounds):
        t_a = timeit(lambda: adamw_step([p], [g], [m], [v], lr=1e-4, beta1=0.9, beta2=0.95, eps=1e-8,
                                        weight_decay=0.1, step=10, out_bf16=[lp]), iters=50)
        t_s = timeit(lambda: sgd_step([p], [g], [m], lr=1e-4, momentum=0.9, weight_decay=1e-4, nesterov=True,
                                      out_bf16=[lp]), iters=50)
        print(json.dumps(dict(tag, n=n, round=rnd, adamw_ms=round(t_a, 4), adamw_GBps=round(n * 28 / t_a / 1e6, 1),
                              sgd_ms=round(t_s, 4), sgd_GBps=round(n * 20 / t_s / 1e6, 1))), flush=True)
    del bases, p, m, v, g, lp
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="41000000,82000000,164000000,328000000")
    ap.add_argument("--offsets", default="", help="element offsets, e.g. 0,1024,16384,262144,1049600,148140")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    torch.manual_seed(0)
    sizes = [int(s) for s in a.sizes.split(",")]
    if a.offsets:
        for off in (int(s) for s in a.offsets.split(",")):
            assert off % 4 == 0 and 4 * off <= PAD
            measure({"offset_elems": off}, sizes[0], a.rounds, off)
    else:
        for n in sizes:
            measure({}, n, a.rounds)


if __name__ == "__main__":
    main()
