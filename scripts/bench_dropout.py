#!/usr/bin/env python
"""Dropout on MI355X: the fused dropout + residual add + LayerNorm site against (1) stock
``torch.nn.functional.dropout`` followed by the existing ``add_norm`` and (2) the plain ``add_norm`` at p = 0,
forward and forward + backward, at the GPT-2 1.3B (98,304 x 2,048) and 124M (65,536 x 768) token shapes, bf16,
p = 0.1; and a GPT-2 124M single-GPU training step at dropout 0.1 against 0.0 and against stock dropout spliced
into the same model.  HIP-event timing, warm-up and repetitions as scripts/bench_kernels.py; the variants alternate
over several rounds in one process and each record carries the median and the range over the rounds.

    python scripts/bench_dropout.py --site-out profiles/dropout_site_vs_composite.jsonl \
        --step-out profiles/gpt2_124m_dropout_step.jsonl
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

DEV = "cuda"
P = 0.1


def timeit(fn, iters=20, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def emit(f, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if f:
        f.write(line + "\n")
        f.flush()


def spread(vals, scale=1.0, nd=1):
    v = sorted(x * scale for x in vals)
    return round(v[len(v) // 2], nd), [round(v[0], nd), round(v[-1], nd)]


def site(rows, N, out, iters, rounds):
    from pytorch_distributedtraining_amd.ops import dropout as D
    from pytorch_distributedtraining_amd.ops.norms import add_norm
    bf = torch.bfloat16
    x = torch.randn(rows, N, device=DEV, dtype=bf, requires_grad=True)
    r = torch.randn(rows, N, device=DEV, dtype=bf, requires_grad=True)
    w = torch.ones(N, device=DEV, dtype=bf, requires_grad=True)
    b = torch.zeros(N, device=DEV, dtype=bf, requires_grad=True)
    rb = torch.zeros(N, device=DEV, dtype=bf, requires_grad=True)
    dy, ds = torch.randn(rows, N, device=DEV, dtype=bf), torch.randn(rows, N, device=DEV, dtype=bf)
    key = D.draw_keys(1, DEV)
    variants = {
        "fused": lambda: add_norm(x, r, w, b, dropout=(P, key, "residual")),
        "fused_rbias": lambda: add_norm(x, r, w, b, r_bias=rb, dropout=(P, key, "residual")),
        "fused_sum_mode": lambda: add_norm(x, r, w, b, dropout=(P, key, "sum")),
        "standalone_kernel_composite": lambda: add_norm(x, D.dropout(r, P, key), w, b),
        "torch_dropout_composite": lambda: add_norm(x, F.dropout(r, P, True), w, b),
        "add_norm_p0": lambda: add_norm(x, r, w, b),
        "add_norm_p0_rbias": lambda: add_norm(x, r, w, b, r_bias=rb),
    }
    stream_bytes = rows * N * 2
    t_f = {name: [] for name in variants}
    t_fb = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            def fwd():
                with torch.no_grad():
                    fn()

            def fwd_bwd():
                # autograd.grad, not .backward(): a gradient returned for two leaves (dx is dr at p = 0 and in sum
                # mode) would be cloned by the second leaf's accumulation, a copy the model never makes
                y, s = fn()
                torch.autograd.grad([y, s], [x, r, w, b], [dy, ds])

            t_f[name].append(timeit(fwd, iters))
            t_fb[name].append(timeit(fwd_bwd, iters))
    for name in variants:
        f_med, f_rng = spread(t_f[name], 1e3)
        fb_med, fb_rng = spread(t_fb[name], 1e3)
        emit(out, {"case": "site", "variant": name, "rows": rows, "N": N, "dtype": "bf16", "p": P, "rounds": rounds,
                   "fwd_us": f_med, "fwd_us_range": f_rng, "fwd_bwd_us": fb_med, "fwd_bwd_us_range": fb_rng,
                   "fwd_GBps_4_streams": round(4 * stream_bytes / f_med / 1e3, 1)})
    del x, r, dy, ds
    torch.cuda.empty_cache()


def _stock_forward(self, input_ids, labels=None):
    """GPT2LMHeadModel.forward with torch's dropout (a stored mask, separate passes) at the same three kinds of
    site, on the norm-side residual adds."""
    p = self._stock_p
    B, S = input_ids.shape
    x = self.wte(input_ids)
    s = F.dropout(x + self.wpe.weight[:S].unsqueeze(0), p, self.training)
    pending = None
    for i, blk in enumerate(self.h):
        if i == 0:
            h, x = blk.ln_1.forward_pass(s)
        else:
            h, x = blk.ln_1.forward_add(x, F.dropout(pending, p, self.training))
        y, x = blk.ln_2.forward_add(x, F.dropout(blk.attn(h), p, self.training))
        pending = blk.mlp(y)
    x, _ = self.ln_f.forward_add(x, F.dropout(pending, p, self.training))
    return self._head(x, labels)


def step(out, batch, seq, steps, warmup, rounds):
    import types

    from pytorch_distributedtraining_amd.models import build_gpt2
    from pytorch_distributedtraining_amd.optim import FusedAdamW
    from pytorch_distributedtraining_amd.parallel.ddp import DistributedDataParallel
    ids = torch.randint(0, 50257, (batch, seq + 1), device=DEV)
    runs = {}
    for variant in ("dropout_0.0", "dropout_0.1_fused", "dropout_0.1_torch"):
        torch.manual_seed(0)
        p = P if variant == "dropout_0.1_fused" else 0.0
        with torch.device(DEV):
            m = build_gpt2("gpt2-124m", embd_pdrop=p, resid_pdrop=p)
        if variant == "dropout_0.1_torch":
            m._stock_p = P
            m.forward = types.MethodType(_stock_forward, m)
        ddp = DistributedDataParallel(m, compute_dtype=torch.bfloat16)
        opt = FusedAdamW(ddp.optimizer_parameters(), lr=1e-4)

        def one(ddp=ddp, opt=opt):
            loss = ddp(ids[:, :-1], labels=ids[:, 1:])
            loss.backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
            return loss

        runs[variant] = one
    times = {v: [] for v in runs}
    peak = {}
    for rnd in range(rounds):
        for variant, one in runs.items():
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            times[variant].append(timeit(one, steps, warmup))
            # the three models are resident together: the step's own peak above what was allocated before it
            peak[variant] = (torch.cuda.max_memory_allocated() - base) / 2**30
    for variant, one in runs.items():
        med, rng = spread(times[variant], 1.0, 2)
        emit(out, {"case": "gpt2-124m step", "variant": variant, "batch": batch, "seq": seq, "rounds": rounds,
                   "ms_per_step": med, "ms_per_step_range": rng, "tokens_per_s": round(batch * seq / med * 1e3),
                   "step_peak_mem_GB": round(peak[variant], 2), "loss": round(float(one().detach()), 4)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--site-out", default=None)
    ap.add_argument("--step-out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seq", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    fs = open(a.site_out, "w") if a.site_out else None
    for rows, N in ((98304, 2048), (65536, 768)):
        site(rows, N, fs, a.iters, a.rounds)
    if not a.skip_step:
        ft = open(a.step_out, "w") if a.step_out else None
        step(ft, a.batch, a.seq, a.steps, a.warmup, a.rounds)


if __name__ == "__main__":
    main()
