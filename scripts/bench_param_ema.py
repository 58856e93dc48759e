#!/usr/bin/env python
"""Parameter EMA on MI355X (the protocol of scripts/bench_drop_path.py: HIP events, the variants alternating over
several rounds in one process, median and [min, max] per record).

1. Kernel: one flat of 41 M, 164 M and 328 M elements (the sizes of profiles/sgd_kernel_vs_adamw_sizes.jsonl), bf16
   gradient and bf16 copy-out: the AdamW and the SGD (momentum, Nesterov) step without the average, with it fused
   (``ema_decay``), and with ``torch._foreach_lerp_`` run after the plain step (what
   ``AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(d))`` runs); and the swap kernel with its bf16 column.
   Bytes per element: AdamW 28, + 8 fused, + 12 composite; SGD 20, + 8 / + 12; swap 18.
2. Step: the SwinIR-S Stoke step (2 micro-batches of 18 LR 128 x 128, MSE, bf16, one GPU, eager) and the GPT-2 124M
   DDP step (16 x 1024, bf16, one GPU): the average off, fused at 0.999, and bolted on with ``AveragedModel`` over the
   Trainer's module; peak memory of each, and one ``averaged_parameters()`` round trip.  ``--baseline`` runs the
   average-off rows alone with nothing but the arguments a tree without the feature knows (for the parent commit;
   ``PDT_BENCH_ROOT=<a built checkout of it>`` makes the script import that tree's package) and appends them.

    python scripts/bench_param_ema.py --kernel-out profiles/param_ema_kernel_vs_composite.jsonl \\
        --step-out profiles/param_ema_step.jsonl
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.environ.get("PDT_BENCH_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

DEV = "cuda"
DECAY = 0.999


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


def kernel(n, out, iters, rounds):
    from pytorch_distributedtraining_amd.ops import adamw_step, sgd_step, swap_
    p, m, v, e = (torch.randn(n, device=DEV) for _ in range(4))
    v.abs_()
    g = torch.randn(n, device=DEV, dtype=torch.bfloat16)
    lp = torch.empty(n, device=DEV, dtype=torch.bfloat16)
    akw = dict(lr=1e-4, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.1, step=10, out_bf16=[lp])
    skw = dict(lr=1e-4, momentum=0.9, weight_decay=1e-4, nesterov=True, out_bf16=[lp])

    def adamw():
        adamw_step([p], [g], [m], [v], **akw)

    def adamw_fused():
        adamw_step([p], [g], [m], [v], emas=[e], ema_decay=DECAY, **akw)

    def adamw_composite():
        adamw_step([p], [g], [m], [v], **akw)
        torch._foreach_lerp_([e], [p], 1.0 - DECAY)

    def sgd():
        sgd_step([p], [g], [m], **skw)

    def sgd_fused():
        sgd_step([p], [g], [m], emas=[e], ema_decay=DECAY, **skw)

    def sgd_composite():
        sgd_step([p], [g], [m], **skw)
        torch._foreach_lerp_([e], [p], 1.0 - DECAY)

    def swap():
        swap_([p], [e], [lp])

    variants = {"adamw": (adamw, 28), "adamw_ema_fused": (adamw_fused, 36), "adamw_ema_foreach_lerp": (adamw_composite, 40),
                "sgd": (sgd, 20), "sgd_ema_fused": (sgd_fused, 28), "sgd_ema_foreach_lerp": (sgd_composite, 32),
                "swap_bf16": (swap, 18)}
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, (fn, _b) in variants.items():
            times[name].append(timeit(fn, iters))
    base = {}
    for name, (_fn, nbytes) in variants.items():
        med, rng = spread(times[name], 1.0, 4)
        rec = {"case": "multi-tensor step, one flat", "variant": name, "n": n, "grad": "bf16", "copy_out": "bf16",
               "rounds": rounds, "launches_per_timing": iters, "ms": med, "ms_range": rng,
               "bytes_per_elem": nbytes, "GBps": round(n * nbytes / med / 1e6, 1)}
        family = name.split("_")[0]
        if name in ("adamw", "sgd"):
            base[family] = med
        elif family in base:
            rec["over_plain_pct"] = round(100.0 * (med / base[family] - 1.0), 1)
        emit(out, rec)
    del p, m, v, e, g, lp
    torch.cuda.empty_cache()


def _swinir(mb):
    from pytorch_distributedtraining_amd.models.swinir import swinir_s_x2
    g = torch.Generator(device=DEV).manual_seed(2000)
    data = [(torch.rand(mb, 3, 128, 128, device=DEV, generator=g), torch.rand(mb, 3, 256, 256, device=DEV, generator=g))
            for _ in range(2)]
    kw = dict(loss=F.mse_loss, batch_size_per_device=mb, grad_accum_steps=2)
    okw = {"lr": 1e-3, "betas": (0.9, 0.99), "eps": 1e-8, "weight_decay": 1e-4}
    return swinir_s_x2, data, kw, okw, 0.1, lambda tr, x, y: tr.loss(tr.model(x), y), 2 * mb


def _gpt2(_mb):
    from pytorch_distributedtraining_amd.models import build_gpt2
    g = torch.Generator(device=DEV).manual_seed(2000)
    t = torch.randint(0, 50257, (16, 1025), device=DEV, generator=g)
    data = [(t[:, :-1], t[:, 1:])]
    kw = dict(loss=lambda out, _tgt: out, batch_size_per_device=16, grad_accum_steps=1)
    okw = {"lr": 1e-4, "betas": (0.9, 0.95), "eps": 1e-8, "weight_decay": 0.1}
    return (lambda: build_gpt2("gpt2-124m", n_positions=1024)), data, kw, okw, 1.0, \
        lambda tr, x, y: tr.loss(tr.model(x, labels=y), y), 16


def step(workload, out, mb, steps, warmup, rounds, baseline):
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

    from pytorch_distributedtraining_amd.trainer import ClipGradNormConfig, StokeOptimizer, Trainer
    build, data, kw, okw, clip, fwd, samples = {"swinir-s-x2 stoke step": _swinir, "gpt2-124m ddp step": _gpt2}[workload](mb)
    specs = {"ema_off": (None, False)} if baseline else {"ema_off": (None, False), "ema_0.999_fused": (DECAY, False),
                                                         "ema_0.999_averaged_model": (None, True)}
    runs, mem = {}, {}
    for variant, (decay, bolt_on) in specs.items():
        torch.manual_seed(0)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        extra = {} if baseline or decay is None else {"param_ema_decay": decay}
        tr = Trainer(build(), optimizer=StokeOptimizer(optimizer=torch.optim.AdamW, optimizer_kwargs=okw),
                     grad_clip=ClipGradNormConfig(max_norm=clip, norm_type=2.0), gpu=True, fp16="bf16",
                     distributed=None, verbose=False, **kw, **extra)
        avg = None
        if bolt_on:     # the utility deep-copies the module it is given: the Trainer's, i.e. its compute copy
            try:
                avg = AveragedModel(tr.model_access, multi_avg_fn=get_ema_multi_avg_fn(DECAY))
            except Exception as exc:  # noqa: BLE001 -- reported as a row, the other variants still run
                emit(out, {"case": workload, "variant": variant, "tree": "this", "error": repr(exc)[:300]})
                continue

        def one(tr=tr, avg=avg):
            for x, y in data:
                loss = fwd(tr, x, y)
                tr.backward(loss)
                if tr.step() and avg is not None:
                    avg.update_parameters(tr.model_access)
            return loss

        one()           # optimizer state (and the average) exist from here on
        torch.cuda.synchronize()
        mem[variant] = {"resident_MB": round((torch.cuda.memory_allocated() - before) / 2 ** 20, 1)}
        runs[variant] = (one, tr)
    times = {v: [] for v in runs}
    for _ in range(rounds):
        for variant, (one, _tr) in runs.items():
            torch.cuda.reset_peak_memory_stats()
            start = torch.cuda.memory_allocated()
            times[variant].append(timeit(one, steps, warmup))
            # the step's own transient memory: the other variants' resident state is in ``start``
            mem[variant]["step_transient_MB"] = round((torch.cuda.max_memory_allocated() - start) / 2 ** 20, 1)
    for variant, (one, tr) in runs.items():
        med, rng = spread(times[variant], 1.0, 2)
        rec = {"case": workload, "variant": variant, "tree": "parent" if baseline else "this", "precision": "bf16",
               "rounds": rounds, "steps_per_timing": steps, "ms_per_step": med, "ms_per_step_range": rng,
               "samples_per_s": round(samples / med * 1e3, 1), **mem[variant],
               "peak_MB": round(mem[variant]["resident_MB"] + mem[variant]["step_transient_MB"], 1),
               "loss": round(float(one().detach()), 5)}
        if variant == "ema_0.999_fused":
            def round_trip(tr=tr):
                with tr.averaged_parameters():
                    pass
            rt = [timeit(round_trip, 10) for _ in range(rounds)]
            rec["averaged_parameters_round_trip_us"], rec["averaged_parameters_round_trip_us_range"] = spread(rt, 1e3)
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
    ap.add_argument("--micro-batch", type=int, default=18)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--baseline", action="store_true",
                    help="the average-off step rows only, without any EMA argument (for a tree without the feature)")
    a = ap.parse_args()
    if not (a.skip_kernel or a.baseline):
        fk = open(a.kernel_out, "w") if a.kernel_out else None
        for n in (int(s) for s in a.sizes.split(",")):
            kernel(n, fk, a.iters, a.rounds)
    if not a.skip_step:
        ft = open(a.step_out, "a" if a.baseline else "w") if a.step_out else None
        for workload in ("swinir-s-x2 stoke step", "gpt2-124m ddp step"):
            step(workload, ft, a.micro_batch, a.steps, a.warmup, a.rounds, a.baseline)


if __name__ == "__main__":
    main()
