#!/usr/bin/env python
"""FusedLAMB on MI355X (the protocol of scripts/bench_param_ema.py: HIP events, 20 launches per timing, the variants
alternating over 5 rounds in one process, median and [min, max] per record).

1. Kernel: one fp32 flat of 41 M, 164 M and 328 M elements cut into GPT-2-like segments (a 50304 x 768 embedding, then
   the twelve tensors of a 768-wide block over and over, every start 16-element aligned), bf16 gradient and bf16
   copy-out: the FusedAdamW step over the flat (one row, what DDP's master gets), the FusedLAMB step (one row per
   segment: stage 1 + row sum + stage 2), and a torch ``_foreach`` LAMB composite over the segment views (foreach
   moments, ``_foreach_norm`` twice, foreach update, one cast).  Bytes per element: AdamW 28, LAMB 40.
2. Step: the GPT-2 124M DDP step (16 x 1024, bf16, one GPU) with AdamW and with LAMB.  ``--baseline`` runs the AdamW row
   alone (for the parent commit; ``PDT_BENCH_ROOT=<a built checkout of it>`` makes the script import that tree's
   package) and appends it.

    python scripts/bench_lamb.py --kernel-out profiles/lamb_kernel_vs_composite.jsonl \\
        --step-out profiles/gpt2_124m_lamb_step.jsonl
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.environ.get("PDT_BENCH_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

DEV = "cuda"
BLOCK = [768, 768, 768 * 2304, 2304, 768 * 768, 768, 768, 768, 768 * 3072, 3072, 3072 * 768, 768]


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


def segments(n):
    """[(start, numel)] filling [0, n): the embedding, then transformer-block tensors, starts 16-aligned."""
    spans, o, k = [], 0, 0
    sizes = [50304 * 768]
    while o < n:
        size = sizes[k] if k < len(sizes) else BLOCK[(k - len(sizes)) % len(BLOCK)]
        size = min(size, n - o)
        spans.append((o, size))
        o = (o + size + 15) // 16 * 16
        k += 1
    return spans


def kernel(n, out, iters, rounds):
    from pytorch_distributedtraining_amd.ops import multi_tensor as mt
    p, m, v = (torch.randn(n, device=DEV) for _ in range(3))
    v.abs_()
    g = torch.randn(n, device=DEV, dtype=torch.bfloat16)
    lp = torch.empty(n, device=DEV, dtype=torch.bfloat16)
    spans = segments(n)
    cut = lambda t: [t[s:s + k] for s, k in spans]
    ps, ms, vs, gs, lps = cut(p), cut(m), cut(v), cut(g), cut(lp)
    b1, b2, eps, wd, lr, t = 0.9, 0.999, 1e-6, 0.01, 1e-4, 10
    bc1, bc2s = 1 - b1 ** t, math.sqrt(1 - b2 ** t)
    akw = dict(lr=lr, beta1=b1, beta2=b2, eps=eps, weight_decay=wd, step=t, out_bf16=[lp])
    sums = torch.zeros(len(spans), 2, device=DEV)
    table = mt.TensorTable([ps, gs, ms, vs, lps])      # built once, as the optimizer's cache keeps them
    gids = list(range(len(spans)))
    lkw = dict(lr=lr, beta1=b1, beta2=b2, eps=eps, weight_decay=wd, step=t, adapt=True, gids=gids,
               n_logical=len(spans), sums=sums, out_bf16=lps, table=table, row_table=mt.RowTable(table, gids))

    def adamw():
        mt.adamw_step([p], [g], [m], [v], **akw)

    def lamb():
        mt.lamb_step(ps, gs, ms, vs, **lkw)

    def composite():
        gv = cut(g.float())
        torch._foreach_mul_(ms, b1)
        torch._foreach_add_(ms, gv, alpha=1 - b1)
        torch._foreach_mul_(vs, b2)
        torch._foreach_addcmul_(vs, gv, gv, value=1 - b2)
        den = torch._foreach_sqrt(vs)
        torch._foreach_div_(den, bc2s)
        torch._foreach_add_(den, eps)
        u = torch._foreach_div(ms, den)
        torch._foreach_div_(u, bc1)
        torch._foreach_add_(u, ps, alpha=wd)
        pn, un = torch._foreach_norm(ps), torch._foreach_norm(u)
        r = (torch.stack(pn) / torch.stack(un) * -lr).unbind(0)
        torch._foreach_mul_(u, r)
        torch._foreach_add_(ps, u)
        lp.copy_(p)

    variants = {"adamw": (adamw, 28), "lamb": (lamb, 40), "lamb_foreach_composite": (composite, None)}
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, (fn, _b) in variants.items():
            times[name].append(timeit(fn, iters))
    base = None
    for name, (_fn, nbytes) in variants.items():
        med, rng = spread(times[name], 1.0, 4)
        rec = {"case": "multi-tensor step, one flat in GPT-2-like segments", "variant": name, "n": n,
               "segments": 1 if name == "adamw" else len(spans), "grad": "bf16", "copy_out": "bf16", "rounds": rounds,
               "launches_per_timing": iters, "ms": med, "ms_range": rng}
        if nbytes is not None:
            rec["bytes_per_elem"] = nbytes
            rec["GBps"] = round(n * nbytes / med / 1e6, 1)
        if name == "adamw":
            base = med
        else:
            rec["over_adamw"] = round(med / base, 3)
        emit(out, rec)
    del p, m, v, g, lp, ps, ms, vs, gs, lps
    torch.cuda.empty_cache()


def step(out, steps, warmup, rounds, baseline):
    from pytorch_distributedtraining_amd.models import build_gpt2
    from pytorch_distributedtraining_amd.trainer import ClipGradNormConfig, StokeOptimizer, Trainer
    gen = torch.Generator(device=DEV).manual_seed(2000)
    tok = torch.randint(0, 50257, (16, 1025), device=DEV, generator=gen)
    x, y = tok[:, :-1], tok[:, 1:]
    specs = {"adamw": (torch.optim.AdamW, {"lr": 1e-4, "betas": (0.9, 0.95), "eps": 1e-8, "weight_decay": 0.1})}
    if not baseline:
        from pytorch_distributedtraining_amd.optim import FusedLAMB
        specs["lamb"] = (FusedLAMB, {"lr": 2e-3, "betas": (0.9, 0.999), "eps": 1e-6, "weight_decay": 0.01})
    runs = {}
    for variant, (cls, okw) in specs.items():
        torch.manual_seed(0)
        tr = Trainer(build_gpt2("gpt2-124m", n_positions=1024),
                     optimizer=StokeOptimizer(optimizer=cls, optimizer_kwargs=okw),
                     grad_clip=ClipGradNormConfig(max_norm=1.0, norm_type=2.0), gpu=True, fp16="bf16",
                     distributed=None, verbose=False, loss=lambda o, _t: o, batch_size_per_device=16,
                     grad_accum_steps=1)

        def one(tr=tr):
            loss = tr.loss(tr.model(x, labels=y), y)
            tr.backward(loss)
            tr.step()
            return loss

        one()           # optimizer state exists from here on
        runs[variant] = (one, tr)
    times = {v: [] for v in runs}
    for _ in range(rounds):
        for variant, (one, _tr) in runs.items():
            times[variant].append(timeit(one, steps, warmup))
    base = None
    for variant, (one, tr) in runs.items():
        med, rng = spread(times[variant], 1.0, 2)
        rec = {"case": "gpt2-124m ddp step", "variant": variant, "tree": "parent" if baseline else "this",
               "precision": "bf16", "optimizer": type(tr.optimizer).__name__, "rounds": rounds,
               "steps_per_timing": steps, "ms_per_step": med, "ms_per_step_range": rng,
               "samples_per_s": round(16 / med * 1e3, 1), "loss": round(float(one().detach()), 5)}
        if variant == "adamw":
            base = med
        else:
            rec["over_adamw"] = round(med / base, 4)
        emit(out, rec)
    del runs
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-out", default=None)
    ap.add_argument("--step-out", default=None)
    ap.add_argument("--sizes", default="41000000,164000000,328000000")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--baseline", action="store_true",
                    help="the AdamW step row only (for a tree without the feature)")
    a = ap.parse_args()
    if not (a.skip_kernel or a.baseline):
        fk = open(a.kernel_out, "w") if a.kernel_out else None
        for n in (int(s) for s in a.sizes.split(",")):
            kernel(n, fk, a.iters, a.rounds)
    if not a.skip_step:
        ft = open(a.step_out, "a" if a.baseline else "w") if a.step_out else None
        step(ft, a.steps, a.warmup, a.rounds, a.baseline)


if __name__ == "__main__":
    main()
