#!/usr/bin/env python
"""ResNet-50 SGD step on one GPU: the Trainer with ``torch.optim.SGD`` mapped to FusedSGD (bf16 compute copy, device
clip coefficient, one multi-tensor launch) against the same Trainer with stock ``torch.optim.SGD`` -- a subclass of
it, which the Trainer never maps (autocast casts, a host sync at every clipped step, torch's foreach step).

Both sides run in this one process, alternating, ``--repeats`` times each; one JSON line per side with the median
samples/s, every run's samples/s and the peak memory."""
import argparse
import gc
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pytorch_distributedtraining_amd import train  # noqa: E402
from pytorch_distributedtraining_amd.run_config import load_config  # noqa: E402


class StockSGD(torch.optim.SGD):
    """torch.optim.SGD under a name of its own: the Trainer keeps a user's subclass as given."""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                     "configs", "resnet50_ddp_sgd.yaml"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--batch-size", type=int, default=None, dest="batch_size_per_device")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    cfg = load_config(a.config, steps=a.steps, batch_size_per_device=a.batch_size_per_device)
    sides = {"fused_sgd": None, "torch_sgd": StockSGD}
    runs = {k: [] for k in sides}
    for _ in range(a.repeats):
        for side, cls in sides.items():
            res = train.run(cfg, optimizer_cls=cls)
            runs[side].append(res)
            gc.collect()
            torch.cuda.empty_cache()
    for side, rs in runs.items():
        rates = [r["samples_per_s"] for r in rs]
        print(json.dumps({"case": f"{cfg.name} 1 GPU, {side}", "model": cfg.model, "batch": cfg.batch_size_per_device,
                          "steps": cfg.steps, "optimizer": cfg.optimizer,
                          "samples_per_s_median": round(statistics.median(rates), 1),
                          "samples_per_s_runs": [round(r, 1) for r in rates],
                          "ms_per_step_median": round(statistics.median(r["ms_per_step"] for r in rs), 2),
                          "peak_mem_gb": max(r["peak_mem_gb"] for r in rs),
                          "loss": rs[-1]["loss"]}), flush=True)


if __name__ == "__main__":
    main()
