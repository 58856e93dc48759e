"""Parameter EMA off the GPU: the CPU branches of the fused steps against torch's ``AveragedModel``, the optimizer
state layout, ZeRO (OSS + ShardedDataParallel) and FSDP over gloo at world 2, the Trainer and the run configuration.

The reference is ``torch.optim.swa_utils.AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(d))`` updated once before
the first step and once after every step, or the same formula in fp64 (``param_ema_ref``)."""
import copy
import dataclasses
import os

import pytest
import torch
import torch.nn as nn
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

from dist_utils import run_workers
from param_ema_ref import Ema64, n_step_bound
from test_fused_sgd_cpu import _data, _model, _shard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 4
ADAMW_KW = dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2)
SGD_KW = dict(lr=1e-2, momentum=0.9, weight_decay=1e-4)
OPTS = {"adamw": (torch.optim.AdamW, ADAMW_KW), "sgd": (torch.optim.SGD, SGD_KW)}


def _fused(name):
    from pytorch_distributedtraining_amd.optim import FusedAdamW, FusedSGD
    return {"adamw": FusedAdamW, "sgd": FusedSGD}[name]


def _averaged(model, decay):
    avg = AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay))
    avg.update_parameters(model)        # once before the first step
    return avg


# ------------------------------------------------------------------------------------------- ops, CPU branches
@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_cpu_step_branch_matches_averaged_model(kind):
    """``adamw_step`` / ``sgd_step`` on CPU tensors with ``emas``: the parameters are bitwise those of the call
    without, the averages are within the n-step bound of an fp64 AveragedModel fed the same fp32 parameters."""
    from pytorch_distributedtraining_amd.ops import multi_tensor as mt
    decay, n = 0.9, 6
    g = torch.Generator().manual_seed(0)
    shapes = [(5,), (33, 17), (1000,)]
    ps = [torch.randn(s, generator=g) for s in shapes]
    qs = [p.clone() for p in ps]
    st = [[torch.zeros_like(p) for p in ps] for _ in range(4)]      # moments / buffers of both runs
    emas = [p.clone() for p in ps]
    holder = nn.ParameterList([nn.Parameter(p.double()) for p in ps])
    avg = _averaged(holder, decay)
    mag = [p.abs().double() for p in ps]
    for s in range(n):
        grads = [torch.randn(sh, generator=g) for sh in shapes]
        if kind == "adamw":
            kw = dict(lr=1e-2, beta1=0.9, beta2=0.99, eps=1e-8, weight_decay=1e-2, step=s + 1)
            mt.adamw_step(ps, grads, st[0], st[1], emas=emas, ema_decay=decay, **kw)
            mt.adamw_step(qs, grads, st[2], st[3], **kw)
        else:
            kw = dict(lr=1e-2, momentum=0.9, weight_decay=1e-4, nesterov=False)
            mt.sgd_step(ps, grads, st[0], emas=emas, ema_decay=decay, **kw)
            mt.sgd_step(qs, grads, st[2], **kw)
        with torch.no_grad():
            for h, p in zip(holder, ps):
                h.copy_(p)
        avg.update_parameters(holder)
        mag = [torch.maximum(m, p.abs().double()) for m, p in zip(mag, ps)]
    for p, q in zip(ps, qs):
        assert torch.equal(p, q)
    for e, a, m in zip(emas, avg.module, mag):
        err = (e.double() - a.detach()).abs()
        assert bool((err <= n_step_bound(n, decay, m)).all()), float(err.max())
    # a skipped step leaves the average alone; rows without an average are left out
    before = [e.clone() for e in emas]
    grads = [torch.randn(sh, generator=g) for sh in shapes]
    flag = torch.ones(1, dtype=torch.int32)
    if kind == "adamw":
        mt.adamw_step(ps, grads, st[0], st[1], emas=emas, ema_decay=decay, found_inf=flag, lr=1e-2, beta1=0.9,
                      beta2=0.99, eps=1e-8, weight_decay=0.0, step=n + 1)
        mt.adamw_step(ps, grads, st[0], st[1], emas=[None, emas[1], None], ema_decay=decay, lr=1e-2, beta1=0.9,
                      beta2=0.99, eps=1e-8, weight_decay=0.0, step=n + 1)
    else:
        mt.sgd_step(ps, grads, st[0], emas=emas, ema_decay=decay, found_inf=flag, lr=1e-2, momentum=0.9,
                    weight_decay=0.0, nesterov=False)
        mt.sgd_step(ps, grads, st[0], emas=[None, emas[1], None], ema_decay=decay, lr=1e-2, momentum=0.9,
                    weight_decay=0.0, nesterov=False)
    assert torch.equal(emas[0], before[0]) and torch.equal(emas[2], before[2])
    assert not torch.equal(emas[1], before[1])


@pytest.mark.parametrize("bad", [0, 1, -0.1, 1.5])
def test_ema_decay_validation(bad):
    from pytorch_distributedtraining_amd.ops import multi_tensor as mt
    p, g, m, v = (torch.zeros(4) for _ in range(4))
    with pytest.raises(ValueError, match="ema_decay"):
        mt.adamw_step([p], [g], [m], [v], lr=1e-3, beta1=0.9, beta2=0.99, eps=1e-8, weight_decay=0.0, step=1,
                      emas=[p.clone()], ema_decay=bad)
    with pytest.raises(ValueError, match="ema_decay"):
        mt.sgd_step([p], [g], [m], lr=1e-3, momentum=0.9, weight_decay=0.0, nesterov=False, emas=[p.clone()],
                    ema_decay=bad)
    for name in OPTS:
        with pytest.raises(ValueError, match="ema_decay"):
            _fused(name)([nn.Parameter(torch.zeros(4))], lr=0.1, ema_decay=bad)
        opt = _fused(name)([nn.Parameter(torch.zeros(4))], lr=0.1, ema_decay=0.5)
        opt.param_groups[0]["ema_decay"] = bad          # the key is read at each step
        opt.param_groups[0]["params"][0].grad = torch.ones(4)
        with pytest.raises(ValueError, match="ema_decay"):
            opt.step()


def test_swap_cpu_and_argument_checks():
    from pytorch_distributedtraining_amd.ops import multi_tensor as mt
    a, b = [torch.randn(7), torch.randn(3, 5)], [torch.randn(7), torch.randn(3, 5)]
    o = [torch.zeros(7, dtype=torch.bfloat16), None]
    a0, b0 = [t.clone() for t in a], [t.clone() for t in b]
    mt.swap_(a, b, o)
    assert all(torch.equal(x, y) for x, y in zip(a, b0)) and all(torch.equal(x, y) for x, y in zip(b, a0))
    assert torch.equal(o[0], a[0].to(torch.bfloat16))
    mt.swap_(a, b, o)
    assert all(torch.equal(x, y) for x, y in zip(a, a0)) and all(torch.equal(x, y) for x, y in zip(b, b0))
    assert torch.equal(o[0], a0[0].to(torch.bfloat16))
    with pytest.raises(ValueError):
        mt.swap_(a, b[:1])
    with pytest.raises(TypeError):
        mt.swap_([a[0].double()], [b[0]])


# ------------------------------------------------------------------------------------------- optimizers
def _train(model, opt, steps, first=0, world=1, after=None):
    for s in range(first, first + steps):
        x, y = _data(s, world)
        opt.zero_grad()
        nn.functional.mse_loss(model(x), y).backward()
        opt.step()
        if after is not None:
            after()


@pytest.mark.parametrize("kind,decay", [("adamw", 0.9), ("sgd", 0.999)])
def test_fused_optimizer_cpu_matches_averaged_model(kind, decay):
    _, kw = OPTS[kind]
    m, twin = _model(), _model()
    opt = _fused(kind)(m.parameters(), ema_decay=decay, **kw)
    plain = _fused(kind)(twin.parameters(), **kw)
    ref64 = copy.deepcopy(m).double()
    avg = _averaged(ref64, decay)
    mag = [p.detach().abs().double() for p in m.parameters()]
    n = 12

    def after():
        with torch.no_grad():
            for r, p in zip(ref64.parameters(), m.parameters()):
                r.copy_(p)
        avg.update_parameters(ref64)
        for i, p in enumerate(m.parameters()):
            mag[i] = torch.maximum(mag[i], p.detach().abs().double())
    _train(m, opt, n, after=after)
    _train(twin, plain, n)
    for p, q in zip(m.parameters(), twin.parameters()):
        assert torch.equal(p, q)                      # the average changes nothing else
    for p, a, mg in zip(m.parameters(), avg.module.parameters(), mag):
        e = opt.state[p]["ema"]
        assert e.dtype == torch.float32 and e.shape == p.shape and e.stride() == p.stride()
        err = (e.double() - a.detach()).abs()
        assert bool((err <= n_step_bound(n, decay, mg)).all()), float(err.max())
        assert not torch.equal(e, p.detach())
    assert all("ema" not in st for st in plain.state_dict()["state"].values())
    assert plain.param_groups[0].get("ema_decay") is None


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_state_dict_moves_to_torch_and_back_and_swap_guard(kind):
    torch_cls, kw = OPTS[kind]
    m = _model()
    opt = _fused(kind)(m.parameters(), ema_decay=0.9, **kw)
    _train(m, opt, 2)
    sd = opt.state_dict()
    assert all("ema" in st for st in sd["state"].values()) and len(sd["state"]) == 6
    assert sd["param_groups"][0]["ema_decay"] == 0.9
    # torch's optimizer carries the unknown state key and keeps stepping
    m2 = copy.deepcopy(m)
    t = torch_cls(m2.parameters(), **kw)
    t.load_state_dict(copy.deepcopy(sd))
    _train(m2, t, 1, first=2)
    assert all("ema" in st for st in t.state_dict()["state"].values())
    # a checkpoint without the key into an optimizer with the average on: it starts at the next step
    m3, m4 = _model(), _model()
    old = _fused(kind)(m3.parameters(), **kw)
    _train(m3, old, 2)
    m4.load_state_dict(m3.state_dict())
    new = _fused(kind)(m4.parameters(), ema_decay=0.9, **kw)
    new.load_state_dict(copy.deepcopy(old.state_dict()))
    assert new.param_groups[0]["ema_decay"] == 0.9 and all("ema" not in st for st in new.state.values())
    before = [p.detach().clone() for p in m4.parameters()]
    _train(m4, new, 1, first=2)
    for p, b in zip(m4.parameters(), before):
        want = b.double() + (1.0 - 0.9) * (p.detach().double() - b.double())
        err = (new.state[p]["ema"].double() - want).abs()
        assert bool((err <= n_step_bound(1, 0.9, torch.maximum(b.abs(), p.detach().abs()))).all())
    # swap: parameters <-> averages, step() refuses meanwhile, the second call restores bit for bit
    ps = [p.detach().clone() for p in m.parameters()]
    es = [opt.state[p]["ema"].clone() for p in m.parameters()]
    assert opt.ema_swapped is False and opt.swap_ema_() == 6 and opt.ema_swapped is True
    assert all(torch.equal(p, e) for p, e in zip(m.parameters(), es))
    assert all(torch.equal(opt.state[p]["ema"], q) for p, q in zip(m.parameters(), ps))
    for p in m.parameters():
        p.grad = torch.zeros_like(p)
    with pytest.raises(RuntimeError, match="swap"):
        opt.step()
    opt.swap_ema_()
    assert opt.ema_swapped is False
    assert all(torch.equal(p, q) for p, q in zip(m.parameters(), ps))
    assert all(torch.equal(opt.state[p]["ema"], e) for p, e in zip(m.parameters(), es))


# ------------------------------------------------------------------------------------------- OSS + SDDP, gloo
DECAY = 0.9


def _reference(kind, world, steps=STEPS):
    """Single process: torch.optim + AveragedModel on the global batch."""
    torch_cls, kw = OPTS[kind]
    m = _model()
    opt = torch_cls(m.parameters(), **kw)
    avg = _averaged(m, DECAY)
    _train(m, opt, steps, world=world, after=lambda: avg.update_parameters(m))
    return [p.detach().clone() for p in avg.module.parameters()], [p.detach().clone() for p in m.parameters()]


def _zero_run(kind, rank, world, swap, **oss_kw):
    from pytorch_distributedtraining_amd.parallel.zero import OSS, ShardedDataParallel
    _, kw = OPTS[kind]
    m = _model()
    opt = OSS(m.parameters(), optim=_fused(kind), ema_decay=DECAY, **oss_kw, **kw)
    model = ShardedDataParallel(m, opt, reduce_buffer_size=256)
    lowp = oss_kw.get("compute_dtype") is not None
    owned = opt.owned_params()
    track = Ema64(owned, DECAY)         # fp64 recursion over this rank's fp32 masters
    for s in range(STEPS):
        x, y = _data(s, world)
        x = _shard(x, rank, world)
        model.zero_grad()
        out = model(x.bfloat16()).float() if lowp else model(x)
        nn.functional.mse_loss(out, _shard(y, rank, world)).backward()
        opt.step()
        track.update(owned)
    assert opt.optim.param_groups[0]["ema_decay"] == DECAY        # through OSS(..., ema_decay=) and _sync_hparams
    track.check([opt.optim.state[p]["ema"] for p in owned], "owned averages")
    # per-rank average memory: the owned parameters' only
    assert sum(st["ema"].numel() for st in opt.optim.state.values()) == sum(p.numel() for p in owned)
    res = {}
    if swap:
        live = [p.detach().clone() for p in m.parameters()]
        opt.swap_ema_()
        assert opt.ema_swapped
        res["swapped"] = [p.detach().float().clone() for p in m.parameters()]
        res["owned_avg"] = {opt._index[id(q)]: track.avg[i] for i, q in enumerate(
            [p for p in opt._all_params if opt._owner_of[id(p)] == rank])}
        with pytest.raises(RuntimeError, match="swap"):
            opt.step()
        opt.swap_ema_()
        assert not opt.ema_swapped
        assert all(torch.equal(a, p.detach()) for a, p in zip(live, m.parameters()))
    # one more step after the round trip (or without it): the swap must leave no trace
    x, y = _data(STEPS, world)
    model.zero_grad()
    x = _shard(x, rank, world)
    out = model(x.bfloat16()).float() if lowp else model(x)
    nn.functional.mse_loss(out, _shard(y, rank, world)).backward()
    opt.step()
    res["final"] = [p.detach().float().clone() for p in m.parameters()]
    res["final_ema"] = [opt.optim.state[p]["ema"].clone() for p in owned]
    opt.consolidate_state_dict(0)
    res["sd"] = opt.state_dict() if rank == 0 else None
    return res


def _zero_mem(kind, rank, world):
    """Bytes of ``"ema"`` tensors this rank holds, on the model of ``test_zero2_gradient_memory`` (eight equal layers:
    the small MLP's largest tensor alone is 59 % of it, so no partition of it meets that test's cap)."""
    from pytorch_distributedtraining_amd.parallel.zero import OSS, ShardedDataParallel
    _, kw = OPTS[kind]
    torch.manual_seed(0)
    m = nn.Sequential(*[nn.Linear(64, 64) for _ in range(8)])
    opt = OSS(m.parameters(), optim=_fused(kind), ema_decay=DECAY, **kw)
    model = ShardedDataParallel(m, opt, reduce_buffer_size=8192)
    model(torch.randn(4, 64)).square().mean().backward()
    opt.step()
    return (sum(st["ema"].numel() * 4 for st in opt.optim.state.values()), sum(p.numel() * 4 for p in m.parameters()))


def _w_zero(rank, world, kind):
    out = {"mem": _zero_mem(kind, rank, world)}
    for mode, oss_kw in (("plain", {}), ("bcast16", {"broadcast_fp16": True}),
                         ("bf16", {"compute_dtype": torch.bfloat16})):
        a = _zero_run(kind, rank, world, True, **oss_kw)
        b = _zero_run(kind, rank, world, False, **oss_kw)
        # a worker that never swapped: bitwise the same parameters and averages
        assert all(torch.equal(x, y) for x, y in zip(a["final"], b["final"])), mode
        assert all(torch.equal(x, y) for x, y in zip(a["final_ema"], b["final_ema"])), mode
        out[mode] = a
    return out


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_oss_sddp_param_ema(kind):
    world = 2
    ref_avg, _ = _reference(kind, world, STEPS + 1)
    at_swap, _ = _reference(kind, world, STEPS)
    outs = run_workers(_w_zero, world, kind)
    for r in outs:      # per-rank average memory: the owned segment only (the cap of test_zero2_gradient_memory)
        ema_bytes, model_bytes = r["mem"]
        assert 0 < ema_bytes <= 0.55 * model_bytes, (ema_bytes, model_bytes)
    for mode in ("plain", "bcast16", "bf16"):
        r0, r1 = outs[0][mode], outs[1][mode]
        sd = r0["sd"]
        assert sorted(sd["state"].keys()) == list(range(6))
        assert all("ema" in sd["state"][i] and sd["state"][i]["ema"].dtype == torch.float32 for i in range(6))
        assert sd["param_groups"][0]["ema_decay"] == DECAY
        # swapped in: every rank holds the owners' averages (exactly; through the 16-bit payload / compute copy in
        # the two low-precision modes, where a peer's replica is the rounding of the owner's fp32 value)
        owned = {**r0["owned_avg"], **r1["owned_avg"]}
        for i in range(6):
            a, b, want = r0["swapped"][i], r1["swapped"][i], owned[i].float().view_as(r0["swapped"][i])
            if mode == "plain":
                assert torch.equal(a, b)
                assert torch.allclose(a, want, atol=2e-5, rtol=0)       # (the bound itself is checked on the owner)
                assert torch.allclose(a, at_swap[i], atol=2e-5), (mode, i)
            elif mode == "bf16":
                assert torch.equal(a, b)
                assert torch.allclose(a, want, atol=1e-7, rtol=2.0 ** -8)
            else:
                assert torch.allclose(a, b, atol=1e-6, rtol=2.0 ** -10)
                assert torch.allclose(a, want, atol=1e-6, rtol=2.0 ** -10)
        if mode == "plain":         # fp32 end to end: the single-process torch.optim + AveragedModel reference
            for i in range(6):
                assert torch.allclose(sd["state"][i]["ema"], ref_avg[i], atol=2e-5), (mode, i)


# ------------------------------------------------------------------------------------------- FSDP, gloo
def _fsdp_build(strategy):
    from pytorch_distributedtraining_amd.optim import FusedAdamW
    from pytorch_distributedtraining_amd.parallel.fsdp import (FullyShardedDataParallel, MixedPrecision,
                                                                ShardingStrategy)
    m = _model()
    eng = FullyShardedDataParallel(m, wrap_classes=(nn.Linear,), sharding_strategy=ShardingStrategy(strategy),
                                   mixed_precision=MixedPrecision(torch.float32, torch.float32),
                                   device=torch.device("cpu"))
    opt = FusedAdamW(eng.flat_parameters(), ema_decay=DECAY, **ADAMW_KW)
    return eng, opt


def _fsdp_step(eng, opt, s, rank, world):
    x, y = _data(s, world)
    opt.zero_grad()
    nn.functional.mse_loss(eng(_shard(x, rank, world)), _shard(y, rank, world)).backward()
    opt.step()


def _w_fsdp(rank, world, strategy):
    eng, opt = _fsdp_build(strategy)
    twin, topt = _fsdp_build(strategy)
    for s in range(STEPS):
        _fsdp_step(eng, opt, s, rank, world)
        _fsdp_step(twin, topt, s, rank, world)
    full = eng.full_optim_state_dict(opt)
    x, _ = _data(99, world)
    with torch.no_grad():
        live_out = eng(x)               # leaves SHARD_GRAD_OP units and the root gathered: swap must drop them
        eng.swap_ema_(opt)
        assert opt.ema_swapped
        avg_out = eng(x)
        avg_sd = eng.state_dict()
        eng.swap_ema_(opt)
        back_out = eng(x)
    assert torch.equal(live_out, back_out)
    _fsdp_step(eng, opt, STEPS, rank, world)
    _fsdp_step(twin, topt, STEPS, rank, world)
    same = all(torch.equal(a, b) for a, b in zip(eng.flat_parameters(), twin.flat_parameters())) and all(
        torch.equal(opt.state[a]["ema"], topt.state[b]["ema"])
        for a, b in zip(eng.flat_parameters(), twin.flat_parameters()))
    # a new engine + optimizer loads the full state: the shards of the average come back
    eng2, opt2 = _fsdp_build(strategy)
    eng2.load_full_optim_state_dict(opt2, full)
    restored = all(torch.equal(opt2.state[b]["ema"], full_shard) for b, full_shard in zip(
        eng2.flat_parameters(), [_reshard(eng2, u, full) for u in eng2.all_units()]))
    return full, avg_out, avg_sd, same, restored


def _reshard(eng, u, full):
    """This rank's shard of unit ``u``'s average, rebuilt from the unflattened full state."""
    idx_of = {f: i for i, f in enumerate(eng._param_fqns)}
    flat = torch.zeros(u.total)
    for (_m, _pn, fqn, _shape), off, n in zip(u.params, u.offsets, u.numels):
        flat[off:off + n] = full["state"][idx_of[fqn]]["ema"].reshape(-1)
    r = eng.comm.rank
    return flat[r * u.shard_numel:(r + 1) * u.shard_numel]


@pytest.mark.parametrize("strategy", ["full_shard", "shard_grad_op"])
def test_fsdp_param_ema(strategy):
    world = 2
    ref_avg, _ = _reference("adamw", world, STEPS)
    outs = run_workers(_w_fsdp, world, strategy)
    full, avg_out, avg_sd, same, restored = outs[0]
    assert same and restored and outs[1][3] and outs[1][4]
    assert sorted(full["state"].keys()) == list(range(6))
    for i in range(6):          # unflattened, under the original indices
        assert full["state"][i]["ema"].shape == ref_avg[i].shape
        assert torch.allclose(full["state"][i]["ema"], ref_avg[i], atol=2e-5), i
    # swapped in, a forward computes with the averaged weights
    ref = _model()
    ref.load_state_dict({k: v for k, v in zip(ref.state_dict().keys(), [full["state"][i]["ema"] for i in range(6)])})
    x, _ = _data(99, world)
    with torch.no_grad():
        want = ref(x)
    assert torch.allclose(avg_out, want, atol=1e-6)
    assert torch.equal(avg_out, outs[1][1])
    for k, v in ref.state_dict().items():
        assert torch.equal(avg_sd[k], v), k


# ------------------------------------------------------------------------------------------- Trainer
def _trainer(opt_cls=torch.optim.AdamW, decay=DECAY, **kw):
    from pytorch_distributedtraining_amd.trainer import StokeOptimizer, Trainer
    okw = dict(SGD_KW) if opt_cls in (torch.optim.SGD,) else dict(lr=1e-2) if opt_cls is torch.optim.RMSprop \
        else dict(ADAMW_KW)
    return Trainer(_model(), StokeOptimizer(optimizer=opt_cls, optimizer_kwargs=okw), loss=nn.functional.mse_loss,
                   batch_size_per_device=8, gpu=False, verbose=False, param_ema_decay=decay, **kw)


def _tr_steps(tr, first, n):
    for s in range(first, first + n):
        x, y = _data(s, 1)
        tr.backward(tr.loss(tr.model(x), y))
        tr.step()


def test_trainer_maps_to_fused_on_cpu_and_rejects_other_optimizers():
    from pytorch_distributedtraining_amd.optim import FusedAdamW, FusedSGD
    tr = _trainer(torch.optim.AdamW)
    assert type(tr.optimizer) is FusedAdamW and tr.optimizer.param_groups[0]["ema_decay"] == DECAY
    assert type(_trainer(torch.optim.SGD).optimizer) is FusedSGD
    assert type(_trainer(torch.optim.AdamW, decay=None).optimizer) is torch.optim.AdamW     # off: as before
    with pytest.raises(ValueError, match="AdamW, Adam or SGD"):
        _trainer(torch.optim.RMSprop)
    with pytest.raises(ValueError, match="param_ema_decay"):
        _trainer(decay=1.0)
    with pytest.raises(RuntimeError, match="param_ema_decay"):
        with _trainer(decay=None).averaged_parameters():
            pass


def test_trainer_averaged_parameters_and_state_dict():
    tr = _trainer()
    _tr_steps(tr, 0, 3)
    live = {k: v.detach().clone() for k, v in tr.model_access.state_dict().items()}
    emas = [tr.optimizer.state[p]["ema"].clone() for p in tr.model_access.parameters()]
    sd = tr.ema_state_dict()
    assert list(sd.keys()) == list(tr._model_state().keys())
    assert all(torch.equal(sd[k], e) for k, e in zip(sd, emas))
    x, y = _data(50, 1)
    tr.eval()
    with tr.averaged_parameters(), torch.no_grad():
        out = tr.model(x)
        with pytest.raises(RuntimeError, match="averaged_parameters"):
            tr.step()
    with pytest.raises(RuntimeError, match="averaged_parameters"):
        with tr.averaged_parameters():
            tr.backward(tr.loss(tr.model(x), y))
    assert not tr.optimizer.ema_swapped                 # swapped out in the finally
    tr.train()
    ref = _model()
    ref.load_state_dict(sd)
    with torch.no_grad():
        assert torch.equal(out, ref(x))
    assert all(torch.equal(v, live[k]) for k, v in tr.model_access.state_dict().items())


def test_trainer_checkpoint_continues_the_average(tmp_path):
    a = _trainer()
    _tr_steps(a, 0, 3)
    path, tag = a.save(str(tmp_path), name="ema")
    _tr_steps(a, 3, 2)
    b = _trainer()
    b.load(path, tag)
    assert all("ema" in st for st in b.optimizer.state.values()) and len(b.optimizer.state) == 6
    _tr_steps(b, 3, 2)
    for p, q in zip(a.model_access.parameters(), b.model_access.parameters()):
        assert torch.equal(p, q)
        assert torch.equal(a.optimizer.state[p]["ema"], b.optimizer.state[q]["ema"])
    assert all(torch.equal(v, w) for v, w in zip(a.ema_state_dict().values(), b.ema_state_dict().values()))


# ------------------------------------------------------------------------------------------- run configuration
def test_run_config_reaches_the_param_groups_and_default_is_off():
    from pytorch_distributedtraining_amd import train
    from pytorch_distributedtraining_amd.optim import FusedAdamW
    from pytorch_distributedtraining_amd.run_config import RunConfig, load_config
    assert RunConfig().ema_decay == 0.0
    cfg = load_config(os.path.join(ROOT, "configs", "resnet18_ddp_cpu.yaml"))
    small = dataclasses.replace(cfg, model="srnet", loss="mse", batch_size_per_device=2, image_size=8, steps=1,
                                warmup=0)
    seen = []
    real_f, real_t = FusedAdamW.step, torch.optim.AdamW.step

    def spy_f(self, *a, **kw):
        r = real_f(self, *a, **kw)
        seen.append(("fused", self.param_groups[0].get("ema_decay"),
                     all("ema" in st for st in self.state_dict()["state"].values())))
        return r

    def spy_t(self, *a, **kw):
        r = real_t(self, *a, **kw)
        seen.append(("torch", self.param_groups[0].get("ema_decay"),
                     any("ema" in st for st in self.state_dict()["state"].values())))
        return r
    FusedAdamW.step, torch.optim.AdamW.step = spy_f, spy_t
    try:
        train.run(dataclasses.replace(small, ema_decay=0.999))
        train.run(small)
    finally:
        FusedAdamW.step, torch.optim.AdamW.step = real_f, real_t
    assert seen == [("fused", 0.999, True), ("torch", None, False)]


def test_swinir_ema_config_differs_in_name_and_decay_only():
    from pytorch_distributedtraining_amd.run_config import load_config
    base = load_config(os.path.join(ROOT, "configs", "swinir_stoke.yaml")).to_dict()
    ema = load_config(os.path.join(ROOT, "configs", "swinir_stoke_ema.yaml")).to_dict()
    diff = {k for k in base if base[k] != ema[k]}
    assert diff == {"name", "ema_decay"} and ema["ema_decay"] == 0.999 and base["ema_decay"] == 0.0
    assert ema["name"] == "swinir_stoke_ema"
