#!/usr/bin/env python
"""Stochastic depth on MI355X (the protocol of scripts/bench_dropout.py: HIP events, the variants alternating over
several rounds in one process, median and [min, max] per record).

1. One SwinIR block's two residual sites -- the window-mapped add + LayerNorm and the fused C = 60 MLP -- at
   18 x 2,048 = 36,864 and 18 x 16,384 = 294,912 rows of 60 channels, bf16, forward and forward + backward:
   the scaled kernels at rate 0.1, the composite (ops.drop_path's standalone kernel, or timm-style torch ops,
   spliced around today's ops) and today's ops at rate 0.
2. The SwinIR-S Stoke step (2 micro-batches of 18 LR 128 x 128, MSE, one GPU, eager): rate 0, rate 0.1 on the fused
   sites, rate 0.1 with the composite forced at both sites, and fp32 at rate 0 and 0.1.  ``--baseline`` runs the
   rate-0 rows alone with nothing but the arguments a tree without stochastic depth knows (for the parent commit;
   ``PDT_BENCH_ROOT=<a built checkout of it>`` makes the script import that tree's package) and appends them.

    python scripts/bench_drop_path.py --site-out profiles/drop_path_site_vs_composite.jsonl \\
        --step-out profiles/swinir_drop_path_step.jsonl
"""
import argparse
import importlib
import json
import os
import sys

sys.path.insert(0, os.environ.get("PDT_BENCH_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

DEV = "cuda"
RATE = 0.1


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


def site(B, H, W, out, iters, rounds):
    from pytorch_distributedtraining_amd.ops import drop_path, drop_path_add
    from pytorch_distributedtraining_amd.ops.norms import add_layer_norm_from_windows
    from pytorch_distributedtraining_amd.ops.swin_mlp import fused_mlp
    DP = importlib.import_module("pytorch_distributedtraining_amd.ops.drop_path")
    bf, C, HID, ws, shift = torch.bfloat16, 60, 120, 8, 4
    rows = B * H * W
    x = torch.randn(B, H * W, C, device=DEV, dtype=bf, requires_grad=True)
    a = torch.randn(rows // (ws * ws), ws * ws, C, device=DEV, dtype=bf, requires_grad=True)
    w = torch.ones(C, device=DEV, dtype=bf, requires_grad=True)
    b = torch.zeros(C, device=DEV, dtype=bf, requires_grad=True)
    w1 = (0.1 * torch.randn(HID, C, device=DEV)).to(bf).requires_grad_()
    b1 = torch.zeros(HID, device=DEV, dtype=bf, requires_grad=True)
    w2 = (0.1 * torch.randn(C, HID, device=DEV)).to(bf).requires_grad_()
    b2 = torch.zeros(C, device=DEV, dtype=bf, requires_grad=True)
    dy = torch.randn(B, H * W, C, device=DEV, dtype=bf)
    keys = torch.tensor([0x0F1E2D3C4B5A6978, -0x1234567], dtype=torch.int64, device=DEV)
    sc = DP.sample_scales(keys, DP.site_table([RATE, RATE], DEV), B)
    sc_a, sc_m = sc[0], sc[1]
    keep = 1.0 - RATE
    m_a, m_m = ((s != 0).to(bf).view(B, 1, 1) for s in (sc_a, sc_m))

    def fused():
        y, s = add_layer_norm_from_windows(x, a, w, b, 1e-5, H, W, ws, shift, sample_scale=sc_a)
        return fused_mlp(y, w1, b1, w2, b2, s, sample_scale=sc_m)

    def composite_kernel():
        y, s = add_layer_norm_from_windows(x, drop_path(a, sc_a), w, b, 1e-5, H, W, ws, shift)
        return drop_path_add(s, fused_mlp(y, w1, b1, w2, b2), sc_m)

    def composite_torch():      # timm's drop_path: x.div(keep) * mask, then the separate residual add
        ad = (a.view(B, -1, C).div(keep) * m_a).view(a.shape)
        y, s = add_layer_norm_from_windows(x, ad, w, b, 1e-5, H, W, ws, shift)
        return s + fused_mlp(y, w1, b1, w2, b2).div(keep) * m_m

    def rate0():
        y, s = add_layer_norm_from_windows(x, a, w, b, 1e-5, H, W, ws, shift)
        return fused_mlp(y, w1, b1, w2, b2, s)

    variants = {"fused_rate_0.1": fused, "composite_kernel_rate_0.1": composite_kernel,
                "composite_torch_rate_0.1": composite_torch, "rate_0": rate0}
    t_f = {name: [] for name in variants}
    t_fb = {name: [] for name in variants}
    leaves = [x, a, w, b, w1, b1, w2, b2]
    for _ in range(rounds):
        for name, fn in variants.items():
            def fwd():
                with torch.no_grad():
                    fn()

            def fwd_bwd():
                torch.autograd.grad([fn()], leaves, [dy])

            t_f[name].append(timeit(fwd, iters))
            t_fb[name].append(timeit(fwd_bwd, iters))
    for name in variants:
        f_med, f_rng = spread(t_f[name], 1e3)
        fb_med, fb_rng = spread(t_fb[name], 1e3)
        emit(out, {"case": "block residual sites", "variant": name, "rows": rows, "C": C, "B": B, "dtype": "bf16",
                   "rate": RATE, "dropped_attn": int((sc_a == 0).sum()), "dropped_mlp": int((sc_m == 0).sum()),
                   "rounds": rounds, "fwd_us": f_med, "fwd_us_range": f_rng, "fwd_bwd_us": fb_med,
                   "fwd_bwd_us_range": fb_rng})
    del x, a, dy
    torch.cuda.empty_cache()


def step(out, mb, steps, warmup, rounds, baseline):
    from pytorch_distributedtraining_amd.models import swinir as S
    from pytorch_distributedtraining_amd.trainer import ClipGradNormConfig, StokeOptimizer, Trainer
    g = torch.Generator(device=DEV).manual_seed(2000)
    data = [(torch.rand(mb, 3, 128, 128, device=DEV, generator=g), torch.rand(mb, 3, 256, 256, device=DEV, generator=g))
            for _ in range(2)]
    if baseline:
        specs = {"rate_0": ("bf16", None, False), "fp32_rate_0": (None, None, False)}
    else:
        specs = {"rate_0": ("bf16", 0.0, False), "rate_0.1_fused": ("bf16", RATE, False),
                 "rate_0.1_composite": ("bf16", RATE, True), "fp32_rate_0": (None, 0.0, False),
                 "fp32_rate_0.1": (None, RATE, False)}
        fused_norm, scaled_ok = S.add_layer_norm_from_windows, S.fused_mlp_scaled_ok

        def composite_norm(x, a_win, weight, bias, eps, H, W, ws, shift, sample_scale=None):
            if sample_scale is not None:
                a_win = S.drop_path(a_win, sample_scale)
            return fused_norm(x, a_win, weight, bias, eps, H, W, ws, shift)

    runs = {}
    for variant, (fp16, rate, composite) in specs.items():
        torch.manual_seed(0)
        model = S.swinir_s_x2() if rate is None else S.swinir_s_x2(drop_path_rate=rate)
        opt = StokeOptimizer(optimizer=torch.optim.AdamW,
                             optimizer_kwargs={"lr": 1e-3, "betas": (0.9, 0.99), "eps": 1e-8, "weight_decay": 1e-4})
        tr = Trainer(model, optimizer=opt, loss=F.mse_loss, batch_size_per_device=mb, grad_accum_steps=2,
                     grad_clip=ClipGradNormConfig(max_norm=0.1, norm_type=2.0), gpu=True, fp16=fp16, distributed=None,
                     verbose=False)

        def one(tr=tr, composite=composite):
            if not baseline:    # both sites through ops.drop_path around today's ops, or on the scaled kernels
                S.add_layer_norm_from_windows = composite_norm if composite else fused_norm
                S.fused_mlp_scaled_ok = (lambda *a: False) if composite else scaled_ok
            for x, y in data:
                loss = tr.loss(tr.model(x), y)
                tr.backward(loss)
                tr.step()
            return loss

        runs[variant] = one
    times = {v: [] for v in runs}
    for _ in range(rounds):
        for variant, one in runs.items():
            times[variant].append(timeit(one, steps, warmup))
    for variant, one in runs.items():
        med, rng = spread(times[variant], 1.0, 2)
        emit(out, {"case": "swinir-s-x2 stoke step", "variant": variant, "tree": "parent" if baseline else "this",
                   "micro_batch": mb, "grad_accum": 2, "image": "3x128x128->3x256x256", "rounds": rounds,
                   "steps_per_timing": steps, "ms_per_step": med, "ms_per_step_range": rng,
                   "samples_per_s": round(2 * mb / med * 1e3, 1), "loss": round(float(one().detach()), 5)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--site-out", default=None)
    ap.add_argument("--step-out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--micro-batch", type=int, default=18)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-site", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--baseline", action="store_true",
                    help="the rate-0 step rows only, without any stochastic-depth argument (for a tree without it)")
    a = ap.parse_args()
    if not (a.skip_site or a.baseline):
        fs = open(a.site_out, "w") if a.site_out else None
        for B, H, W in ((18, 32, 64), (18, 128, 128)):
            site(B, H, W, fs, a.iters, a.rounds)
    if not a.skip_step:
        ft = open(a.step_out, "a" if a.baseline else "w") if a.step_out else None
        step(ft, a.micro_batch, a.steps, a.warmup, a.rounds, a.baseline)


if __name__ == "__main__":
    main()
