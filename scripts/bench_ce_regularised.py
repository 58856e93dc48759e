#!/usr/bin/env python
"""Label smoothing / z-loss inside the cross-entropy kernels on MI355X: the LM heads' call
(``cross_entropy(..., inplace_backward=True, grad_in_forward=True)`` + backward) plain, with ``label_smoothing=0.1``,
with ``z_loss=1e-4`` and with both, against the torch composite
``F.cross_entropy(x.float(), t, label_smoothing=) + z * logsumexp(x.float())^2`` (mean over the rows), bf16 logits at
98,304 x 50,304 (the flagship: fused forward + gradient kernel), 16,384 x 50,304 and 32,768 x 128,256 (Llama-3: the
two-pass kernels); and a GPT-2 124M single-GPU DDP training step with both terms against the plain loss.

Protocol of scripts/bench_dropout.py: HIP events, 20 calls per timing after a warm-up, the variants alternating over
5 rounds in one process, median [min, max] over the rounds.  ``--parent-root DIR`` (a built checkout of the parent
commit) adds the plain call measured alone in a process of its own, on that tree and on this one, once before and
once after this tree's rounds, for the one timing condition: the plain path must not regress.

The in-place kernels overwrite the logits with their gradient, so from the second call on the "logits" are the
previous call's gradient values; the kernels' work does not depend on the values.

    python scripts/bench_ce_regularised.py --out profiles/ce_regularised_vs_composite.jsonl \
        --step-out profiles/gpt2_124m_ce_regularised_step.jsonl [--parent-root ../parent]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--step-out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seq", type=int, default=1024)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-composite", action="store_true")
    ap.add_argument("--parent-root", default=None, help="built checkout of the parent commit (plain path A/B)")
    ap.add_argument("--plain-only", default=None, metavar="LABEL",
                    help="time only the plain call, importing the package from --pkg-root (the parent's process)")
    ap.add_argument("--pkg-root", default=ROOT)
    return ap.parse_args()


A = _args()
sys.path.insert(0, os.path.abspath(A.pkg_root))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

DEV = "cuda"
SHAPES = ((98304, 50304), (16384, 50304), (32768, 128256))
EPS, Z = 0.1, 1e-4


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


def composite(x, t, eps, z):
    xf = x.float()
    loss = F.cross_entropy(xf, t, label_smoothing=eps)
    return loss + z * torch.logsumexp(xf, -1).square().mean() if z else loss


def kernels(rows, V, out, iters, rounds, plain_only=None, skip_composite=False):
    from pytorch_distributedtraining_amd.ops import cross_entropy
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(rows, V, device=DEV, dtype=torch.bfloat16, generator=g).requires_grad_()
    t = torch.randint(0, V, (rows,), device=DEV, generator=g)

    def head(**kw):
        def run():
            loss = cross_entropy(x, t, inplace_backward=True, grad_in_forward=True, **kw)
            torch.autograd.grad(loss, x)        # the gradient is the logits buffer itself: nothing is accumulated
        return run

    def torch_composite(eps, z):
        def run():
            torch.autograd.grad(composite(x, t, eps, z), x)
        return run

    if plain_only:
        variants = {plain_only: head()}
    else:
        variants = {"plain": head(), "eps_0.1": head(label_smoothing=EPS), "z_1e-4": head(z_loss=Z),
                    "eps_0.1_z_1e-4": head(label_smoothing=EPS, z_loss=Z)}
        if not skip_composite:
            variants["torch_composite_plain"] = torch_composite(0.0, 0.0)
            variants["torch_composite_eps_0.1_z_1e-4"] = torch_composite(EPS, Z)
    times = {n: [] for n in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(timeit(fn, iters))
    path = "fused fwd+grad" if V <= 65536 else "two-pass"
    for name in variants:
        med, rng = spread(times[name], 1e3)
        emit(out, {"case": "cross_entropy fwd+bwd", "variant": name, "rows": rows, "V": V, "dtype": "bf16",
                   "path": "torch" if name.startswith("torch") else path, "rounds": rounds, "iters": iters,
                   "us": med, "us_range": rng, "logits_GB": round(rows * V * 2 / 1e9, 2)})
    del x
    torch.cuda.empty_cache()


def parent_plain(root, label, out, a):
    """The plain call on another checkout, in a process of its own (this script, importing that tree's package)."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-only", label, "--pkg-root", root,
                        "--iters", str(a.iters), "--rounds", str(a.rounds)], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"parent-tree run failed:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            emit(out, json.loads(line))


def step(out, batch, seq, steps, warmup, rounds):
    from pytorch_distributedtraining_amd.models import build_gpt2
    from pytorch_distributedtraining_amd.optim import FusedAdamW
    from pytorch_distributedtraining_amd.parallel.ddp import DistributedDataParallel
    ids = torch.randint(0, 50257, (batch, seq + 1), device=DEV)
    runs = {}
    for variant, kw in (("off", {}), ("eps_0.1_z_1e-4", dict(label_smoothing=EPS, z_loss=Z))):
        torch.manual_seed(0)
        with torch.device(DEV):
            m = build_gpt2("gpt2-124m", **kw)
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
    for _ in range(rounds):
        for variant, one in runs.items():
            times[variant].append(timeit(one, steps, warmup))
    for variant, one in runs.items():
        med, rng = spread(times[variant], 1.0, 2)
        emit(out, {"case": "gpt2-124m step", "variant": variant, "batch": batch, "seq": seq, "rounds": rounds,
                   "ms_per_step": med, "ms_per_step_range": rng, "tokens_per_s": round(batch * seq / med * 1e3),
                   "loss": round(float(one().detach()), 4)})


def main(a):
    if not torch.cuda.is_available():
        raise SystemExit("bench_ce_regularised.py measures on a GPU; none found")
    if a.plain_only:
        import pytorch_distributedtraining_amd as pkg
        assert os.path.abspath(pkg.__file__).startswith(os.path.abspath(a.pkg_root) + os.sep), pkg.__file__
        for rows, V in SHAPES:
            kernels(rows, V, None, a.iters, a.rounds, plain_only=a.plain_only)
        return
    f = open(a.out, "w") if a.out else None
    # like with like: the plain call alone in a process of its own, on the parent commit and on this tree, before
    # and after the rounds in which it alternates with the other variants (the composite's 20-60 GB of temporaries)
    if a.parent_root:
        parent_plain(a.parent_root, "plain_parent_commit_before", f, a)
        parent_plain(ROOT, "plain_own_process_before", f, a)
    for rows, V in SHAPES:
        kernels(rows, V, f, a.iters, a.rounds, skip_composite=a.skip_composite)
    if a.parent_root:
        parent_plain(ROOT, "plain_own_process_after", f, a)
        parent_plain(a.parent_root, "plain_parent_commit_after", f, a)
    if not a.skip_step:
        ft = open(a.step_out, "w") if a.step_out else None
        step(ft, a.batch, a.seq, a.steps, a.warmup, a.rounds)


if __name__ == "__main__":
    main(A)
