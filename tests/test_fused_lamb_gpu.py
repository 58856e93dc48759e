"""FusedLAMB on the GPU: the two stage kernels and the row sum against the fp64 definition (tests/lamb_ref.py) on every
kernel path, segmented flats, bitwise reproducibility, found_inf / grad_scale, zero norms, graph capture, the Trainer's
compute-copy path and FSDP at world 2 on one GPU."""
import copy

import pytest
import torch
import torch.nn as nn

import lamb_ref
from dist_utils import assert_adam_close, run_workers
from sgd_cases import clones, tensor_list

pytestmark = pytest.mark.gpu
DEV = "cuda"
EDGE = [1, 32767, 32768, 32769]       # around DEFAULT_CHUNK
MANY = 300                            # one-block rows: the row sum's indexing


def _tensors(seed=0):
    """sgd_cases' list (every vector / tail / scalar path) + the chunk boundary + many one-block rows."""
    g = torch.Generator().manual_seed(1000 + seed)
    extra = [torch.randn(n, generator=g) for n in EDGE] + [torch.randn(7, generator=g) for _ in range(MANY)]
    return tensor_list(DEV, seed=seed) + [t.to(DEV) for t in extra]


def _set_grads(ps, gs, gdt, scale=1.0):
    for p, g in zip(ps, gs):
        if gdt == torch.float32:
            p.grad = (g * scale).reshape(p.shape)
        else:
            p._pdt_grad = (g * scale).to(gdt).reshape(p.shape)   # low-precision grad next to an fp32 master


def _got(ps, opt):
    return ([p.detach() for p in ps], [opt.state[p]["exp_avg"] for p in ps],
            [opt.state[p]["exp_avg_sq"] for p in ps], opt.trust_sums[0])


def _maxdiff(a, b):
    return (a.detach().float() - b.detach().float()).abs().max().item()


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16])
def test_kernels_match_fp64_reference(gdt, wd):
    from pytorch_distributedtraining_amd.optim import FusedLAMB
    ts = _tensors()
    grads = [[g.to(gdt).float() for g in _tensors(seed=10 + s)] for s in range(5)]
    kw = dict(lr=1e-2, weight_decay=wd)
    ref, comp = lamb_ref.reference_and_composite(ts, grads, **kw)
    ps = clones(ts)
    assert ps[4].data_ptr() % 16 == 4          # the misaligned tensor stays misaligned
    opt = FusedLAMB(ps, **kw)
    for gl in grads:
        _set_grads(ps, gl, gdt)
        opt.step()
    assert opt.trust_sums[0].shape == (len(ts), 2) and opt.trust_sums[0].is_cuda
    lamb_ref.check(_got(ps, opt), ref, comp, f"gpu {gdt} wd={wd}")
    if wd == 0:       # no adaptation: the sums are still reported
        assert float(opt.trust_sums[0].min()) > 0


# spans at multiples of 16: one crossing a chunk boundary (40,000 > 32,768 from its start), one of 1 element, gaps
# [0, 16), [40016, 40032), [40033, 40064) and [69064, 70000)
SPANS = [(16, 40000, 0), (40032, 1, 1), (40064, 29000, 2)]
FLAT_N = 70000


def test_segmented_flat_matches_separate_tensors_bitwise():
    from pytorch_distributedtraining_amd.optim import FusedLAMB
    from pytorch_distributedtraining_amd.parallel._segments import Segments
    g = torch.Generator(device=DEV).manual_seed(7)
    init = torch.randn(FLAT_N, device=DEV, generator=g)
    flat = nn.Parameter(init.clone())
    flat._pdt_segments = Segments(SPANS, len(SPANS), None)
    flat._pdt_lp_shard = init.to(torch.bfloat16)
    flat._pdt_grad = torch.zeros(FLAT_N, dtype=torch.bfloat16, device=DEV)
    lp0 = flat._pdt_lp_shard.clone()
    parts = [nn.Parameter(init[s:s + n].clone()) for s, n, _ in SPANS]
    for p, (s, n, _) in zip(parts, SPANS):
        p._pdt_lp_shard = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
        p._pdt_grad = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    kw = dict(lr=1e-2, weight_decay=0.01, ema_decay=0.9)
    o1, o2 = FusedLAMB([flat], **kw), FusedLAMB(parts, **kw)
    gap = torch.ones(FLAT_N, dtype=torch.bool, device=DEV)
    for s, n, _ in SPANS:
        gap[s:s + n] = False
    for k in range(3):
        gr = torch.randn(FLAT_N, device=DEV, generator=g).to(torch.bfloat16)
        flat._pdt_grad.copy_(gr)
        for p, (s, n, _) in zip(parts, SPANS):
            p._pdt_grad.copy_(gr[s:s + n])
        o1.step()
        o2.step()
        if k == 0:      # poison the gaps of the state: "kept their bits" must not mean "stayed zero"
            for key in ("exp_avg", "exp_avg_sq", "ema"):
                o1.state[flat][key][gap] = 7.25
    st = o1.state[flat]
    assert st["exp_avg"].shape == st["ema"].shape == flat.shape
    for p, (s, n, _) in zip(parts, SPANS):
        assert torch.equal(flat.detach()[s:s + n], p.detach())
        for key in ("exp_avg", "exp_avg_sq", "ema"):
            assert torch.equal(st[key][s:s + n], o2.state[p][key]), key
        assert torch.equal(flat._pdt_lp_shard[s:s + n], flat.detach()[s:s + n].bfloat16())
        assert torch.equal(flat._pdt_lp_shard[s:s + n], p._pdt_lp_shard)
    assert torch.equal(o1.trust_sums[0], o2.trust_sums[0])
    assert torch.equal(flat.detach()[gap], init[gap]) and torch.equal(flat._pdt_lp_shard[gap], lp0[gap])
    for key in ("exp_avg", "exp_avg_sq", "ema"):
        assert bool((st[key][gap] == 7.25).all()), key


def test_step_is_bitwise_reproducible():
    from pytorch_distributedtraining_amd.optim import FusedLAMB
    ts = _tensors()
    runs = []
    for _ in range(2):
        ps = clones(ts)
        opt = FusedLAMB(ps, lr=1e-2)
        for s in range(3):
            _set_grads(ps, _tensors(seed=20 + s), torch.bfloat16)
            opt.step()
        runs.append(([p.detach().clone() for p in ps], opt.trust_sums[0].clone()))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    assert torch.equal(runs[0][1], runs[1][1])


def test_found_inf_and_grad_scale():
    from pytorch_distributedtraining_amd.optim import FusedLAMB
    ts = tensor_list(DEV)
    kw = dict(lr=1e-2, weight_decay=0.01, ema_decay=0.9)
    p1, p2 = clones(ts), clones(ts)
    for p in p1:
        p._pdt_lp_shard = p.detach().to(torch.bfloat16)
    o1, o2 = FusedLAMB(p1, **kw), FusedLAMB(p2, **kw)
    quarter = torch.full((1,), 0.25, device=DEV)
    for s in range(2):
        gs = tensor_list(DEV, seed=40 + s)
        _set_grads(p1, gs, torch.float32, scale=4.0)
        _set_grads(p2, gs, torch.float32)
        o1.step(grad_scale=quarter)
        o2.step()
    for a, b in zip(p1, p2):
        assert _maxdiff(a, b) <= 1e-6
        assert _maxdiff(o1.state[a]["exp_avg"], o2.state[b]["exp_avg"]) <= 1e-6
        assert _maxdiff(o1.state[a]["exp_avg_sq"], o2.state[b]["exp_avg_sq"]) <= 1e-6
    state = lambda: [t.clone() for p in p1 for t in (p.detach(), o1.state[p]["exp_avg"], o1.state[p]["exp_avg_sq"],
                                                     o1.state[p]["ema"], o1.state[p]["step"], p._pdt_lp_shard)]
    before = state()
    assert o1.state[p1[0]]["step"].is_cuda and float(o1.state[p1[0]]["step"]) == 2.0
    o1.step(found_inf=torch.ones(1, dtype=torch.int32, device=DEV))
    assert all(torch.equal(a, b) for a, b in zip(before, state()))
    o1.step(found_inf=torch.zeros(1, dtype=torch.int32, device=DEV))
    assert not any(torch.equal(a, b) for a, b in zip(before, state()))
    assert float(o1.state[p1[0]]["step"]) == 3.0


def test_zero_norms():
    from pytorch_distributedtraining_amd.optim import FusedLAMB
    g = torch.Generator().manual_seed(3)
    z, gz = [torch.zeros(37, device=DEV)], [[torch.randn(37, generator=g).to(DEV)]]
    ref, comp = lamb_ref.reference_and_composite(z, gz, lr=1e-2, weight_decay=0.01)
    ps = clones(z)
    opt = FusedLAMB(ps, lr=1e-2, weight_decay=0.01)
    _set_grads(ps, gz[0], torch.float32)
    opt.step()
    assert float(opt.trust_sums[0][0, 0]) == 0.0 and float(opt.trust_sums[0][0, 1]) > 0
    assert torch.isfinite(ps[0]).all() and float(ps[0].detach().abs().max()) > 0
    lamb_ref.check(_got(ps, opt), ref, comp, "gpu zero parameter")
    t, g0 = [torch.randn(37, generator=g).to(DEV)], [[torch.zeros(37, device=DEV)]]
    kw = dict(lr=1e-2, weight_decay=0.0, always_adapt=True)
    ref, comp = lamb_ref.reference_and_composite(t, g0, **kw)
    ps = clones(t)
    opt = FusedLAMB(ps, **kw)
    _set_grads(ps, g0[0], torch.float32)
    opt.step()
    assert float(opt.trust_sums[0][0, 1]) == 0.0 and float(opt.trust_sums[0][0, 0]) > 0
    assert torch.equal(ps[0].detach(), t[0]) and torch.isfinite(opt.state[ps[0]]["exp_avg_sq"]).all()
    lamb_ref.check(_got(ps, opt), ref, comp, "gpu zero gradient")


def test_graph_capture_advances_the_bias_corrections():
    from pytorch_distributedtraining_amd.optim import FusedLAMB
    ts, gs = tensor_list(DEV), tensor_list(DEV, seed=50)
    kw = dict(lr=1e-2, weight_decay=0.01)
    ref, comp = lamb_ref.reference_and_composite(ts, [gs] * 3, **kw)
    ps = clones(ts)
    opt = FusedLAMB(ps, capturable=True, **kw)
    _set_grads(ps, gs, torch.float32)            # fixed gradient buffers
    # warm-up: a skipped step creates the state, the device tables and the sums and, by design, changes nothing
    opt.step(found_inf=torch.ones(1, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    assert all(torch.equal(a.detach(), t) for a, t in zip(ps, ts))      # capturing runs nothing
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert float(opt.state[ps[0]]["step"]) == 3.0
    lamb_ref.check(_got(ps, opt), ref, comp, "gpu graph replay")
    # ... which three eager steps give as well
    qs = clones(ts)
    eager = FusedLAMB(qs, **kw)
    _set_grads(qs, gs, torch.float32)
    for _ in range(3):
        eager.step()
    lamb_ref.check(_got(qs, eager), ref, comp, "gpu eager")


# ------------------------------------------------------------------------------------------------------ Trainer
LAMB_KW = {"lr": 1e-3, "weight_decay": 0.01}


def _tiny():
    from pytorch_distributedtraining_amd.models import build_gpt2
    torch.manual_seed(0)
    return build_gpt2("gpt2-tiny")


def _trainer(model, gpu):
    from pytorch_distributedtraining_amd.optim import FusedLAMB
    from pytorch_distributedtraining_amd.trainer import ClipGradNormConfig, StokeOptimizer, Trainer
    return Trainer(model, optimizer=StokeOptimizer(optimizer=FusedLAMB, optimizer_kwargs=dict(LAMB_KW)),
                   loss=lambda out, tgt: out, batch_size_per_device=4,
                   grad_clip=ClipGradNormConfig(max_norm=1.0, norm_type=2.0), gpu=gpu, fp16="bf16" if gpu else None,
                   distributed=None, verbose=False)


def _tokens(n):
    g = torch.Generator().manual_seed(3)
    return [torch.randint(0, 512, (4, 65), generator=g) for _ in range(n)]


def test_trainer_fused_lamb_with_compute_copy():
    """The fp32 master after 2 Trainer steps against a CPU fp32 run of FusedLAMB's torch-op path over per-tensor copies
    of the same model, stepped with the engine's own (bf16) gradients and torch's clip -- the hand loop and the 1e-5 of
    test_trainer_maps_sgd_to_fused_sgd_with_compute_copy -- and against an independent CPU fp32 Trainer run of the
    same model and seed, where bf16 gradients may flip the sign of near-zero components: the bulk agrees and every
    element stays within the displacement bound (dist_utils.assert_adam_close, |r u| <= 1 here)."""
    from pytorch_distributedtraining_amd.optim import FusedLAMB
    from pytorch_distributedtraining_amd.optim._grads import grad_of
    base = _tiny()
    n_params = len(list(base.parameters()))
    tr = _trainer(copy.deepcopy(base), gpu=True)
    assert type(tr.optimizer) is FusedLAMB and tr.compute_dtype == torch.bfloat16
    assert type(tr._engine).__name__ == "DistributedDataParallel"
    masters = list(tr._clip_params())
    assert len(masters) == 1 and masters[0].dtype == torch.float32
    master = masters[0]
    seg = master._pdt_segments
    assert seg.comm is None and seg.n_logical == len(seg.spans) == n_params
    ref = [nn.Parameter(master.detach()[s:s + n].cpu().clone()) for s, n, _ in seg.spans]
    ropt = FusedLAMB(ref, **LAMB_KW)
    cpu = _trainer(copy.deepcopy(base), gpu=False)
    for x in _tokens(2):
        xd = x.to(DEV)
        tr.backward(tr.loss(tr.model(xd[:, :-1], labels=xd[:, 1:]), None))
        g = grad_of(master).detach().float().cpu()
        for r, (s, n, _) in zip(ref, seg.spans):
            r.grad = g[s:s + n].clone()
        torch.nn.utils.clip_grad_norm_(ref, 1.0)
        ropt.step()
        assert tr.step()
        cpu.backward(cpu.loss(cpu.model(x[:, :-1], labels=x[:, 1:]), None))
        assert cpu.step()
    sums = tr.optimizer.trust_sums[0]
    assert sums.shape == (n_params, 2) and float(sums.min()) > 0
    assert torch.equal(master._pdt_lp_shard, master.detach().bfloat16())
    lp_of = {id(p): p for p in tr.model_access.parameters()}
    assert all(p.dtype == torch.bfloat16 and p.untyped_storage().data_ptr() ==
               master._pdt_lp_shard.untyped_storage().data_ptr() for p in lp_of.values())
    worst = 0.0
    for r, (s, n, _) in zip(ref, seg.spans):
        worst = max(worst, _maxdiff(r, master.detach()[s:s + n].cpu()))
    print("master vs hand loop", worst)
    assert worst < 1e-5
    torch.testing.assert_close(sums.cpu(), ropt.trust_sums[0], rtol=1e-4, atol=0)       # span i is tensor i
    sd_g = {k: v.float().cpu() for k, v in tr.model_access.state_dict().items() if v.is_floating_point()}
    sd_c = {k: v.float() for k, v in cpu.model_access.state_dict().items() if v.is_floating_point()}
    assert_adam_close(sd_c, sd_g, lr=LAMB_KW["lr"], steps=2)


class _Net(nn.Module):
    """Conv + BatchNorm + Linear: under the compute copy a bf16 and an fp32 (batch norm) flat master in one group."""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 8, 3, padding=1, bias=False)
        self.bn = nn.BatchNorm2d(8)
        self.fc = nn.Linear(8, 10)

    def forward(self, x):
        return self.fc(torch.relu(self.bn(self.conv(x))).mean((2, 3)))


def test_trainer_graph_with_fused_lamb_matches_eager():
    """Trainer.graph switches FusedLAMB to its device step count (as FusedAdamW); five graphed steps (2 warm-up,
    capture + replay, 2 replays) against five eager ones, to the bounds test_trainer_graph_with_fused_sgd_matches_eager
    uses.  Two flat masters (bf16 and batch-norm fp32 groups) share the group's sums."""
    from pytorch_distributedtraining_amd.optim import FusedLAMB
    from pytorch_distributedtraining_amd.trainer import ClipGradNormConfig, StokeOptimizer, Trainer
    torch.manual_seed(0)
    base = _Net()
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn(4, 3, 16, 16, device=DEV, generator=g)
    y = torch.randint(0, 10, (4,), device=DEV, generator=g)

    def make():
        tr = Trainer(copy.deepcopy(base), optimizer=StokeOptimizer(optimizer=FusedLAMB, optimizer_kwargs=dict(LAMB_KW)),
                     loss=lambda out, tgt: nn.functional.cross_entropy(out.float(), tgt), batch_size_per_device=4,
                     grad_clip=ClipGradNormConfig(max_norm=1.0, norm_type=2.0), gpu=True, fp16="bf16",
                     distributed=None, verbose=False)

        def step():
            tr.backward(tr.loss(tr.model(x), y))
            tr.step()
        return tr, step

    tr_e, step_e = make()
    for _ in range(5):
        step_e()
    tr_g, step_g = make()
    run = tr_g.graph(step_g, warmup=2)
    for _ in range(3):
        run()
    assert tr_g.optimizer_steps == tr_e.optimizer_steps == 5
    masters = list(tr_g._clip_params())
    assert len(masters) == 2 and all(hasattr(m, "_pdt_segments") for m in masters)
    assert tr_g.optimizer.param_groups[0]["capturable"] is True
    assert all(float(tr_g.optimizer.state[m]["step"]) == 5.0 for m in masters)
    assert tr_g.optimizer.trust_sums[0].shape == (len(list(base.parameters())), 2)
    ema_e, ema_g = float(tr_e._ema), float(tr_g._ema)
    assert abs(ema_g - ema_e) < 2e-3 * max(1.0, abs(ema_e)), (ema_e, ema_g)
    se, sg = tr_e.model_access.state_dict(), tr_g.model_access.state_dict()
    for k in se:
        if se[k].is_floating_point() and se[k].dim() >= 2:
            d = (se[k].float() - sg[k].float()).abs().mean().item()
            assert d < 1e-4, (k, d)


# ------------------------------------------------------------------------------------------------------ FSDP
def _train_fsdp(rank, world, steps):
    from pytorch_distributedtraining_amd.models import build_gpt2
    from pytorch_distributedtraining_amd.optim import FusedLAMB, clip_grad_norm_
    from pytorch_distributedtraining_amd.parallel import Comm, FullyShardedDataParallel
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    with torch.device(dev):
        m = build_gpt2("gpt2-tiny", n_embd=256, n_head=2, n_layer=2)
    comm = Comm()
    f = FullyShardedDataParallel(m, comm=comm, device=dev, keep_low_precision_grads=True)
    opt = FusedLAMB(f.flat_parameters(), lr=1e-3)
    cut = sum(len(p._pdt_segments.spans) for p in f.flat_parameters())
    losses = []
    for s in range(steps):
        g = torch.Generator().manual_seed(s)
        x = torch.randint(0, 512, (4, 129), generator=g).to(dev)
        n = x.shape[0] // world
        xs = x[rank * n:(rank + 1) * n]
        loss = f(xs[:, :-1], labels=xs[:, 1:])
        loss.backward()
        _, coef, _ = clip_grad_norm_(f.flat_parameters(), 1.0, comm=comm, sharded=True, apply=False)
        opt.step(grad_scale=coef)
        opt.zero_grad()
        t = loss.detach().reshape(1).clone()
        comm.all_reduce(t, "avg")
        losses.append(float(t.item()))
    sd = {k: v.float().cpu() for k, v in f.state_dict().items()}
    return losses, sd, opt.trust_sums[0].cpu(), cut


def test_fsdp_two_ranks_on_one_gpu_matches_one_rank():
    (l1, sd1, s1, c1), = run_workers(_train_fsdp, 1, 3)
    (l2, sd2, s2, c2), (l2b, _, s2b, c2b) = run_workers(_train_fsdp, 2, 3)
    assert l2 == l2b
    assert c2 + c2b > c1            # tensors cut by the rank boundary have a span on both ranks
    for a, b in zip(l1, l2):
        assert abs(a - b) < 2e-2 * abs(a)
    assert torch.equal(s2, s2b)     # the all-reduced norms: every rank forms the same ratios
    # ||p||^2 of whole tensors, not of shards (half of it for a cut tensor).  Compared on the tensors that start
    # non-zero: a zero-initialised bias holds nothing but two sign-sensitive updates of size ~lr
    big = s1[:, 0] > 1.0
    assert int(big.sum()) >= 8
    torch.testing.assert_close(s2[big, 0], s1[big, 0], rtol=1e-3, atol=0)
    # the k third of the qkv bias has an exactly-zero gradient (softmax shift invariance): noise-driven steps
    assert_adam_close(sd1, sd2, zero_grad_slices={"attn.c_attn.bias": slice(256, 512)})
