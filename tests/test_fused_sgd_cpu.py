"""FusedSGD off the GPU: its CPU reference path against torch.optim.SGD, ZeRO (OSS + ShardedDataParallel) over
gloo at world 2, and the ``name: sgd`` run configuration."""
import dataclasses
import os

import pytest
import torch
import torch.nn as nn

from dist_utils import run_workers
from sgd_cases import clones, tensor_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 3


@pytest.mark.parametrize("momentum,nesterov", [(0.9, False), (0.9, True), (0.0, False)])
@pytest.mark.parametrize("wd", [0.0, 1e-4])
def test_fused_sgd_cpu_matches_torch(momentum, nesterov, wd):
    from pytorch_distributedtraining_amd.optim import FusedSGD
    ts = tensor_list()
    p1, p2 = clones(ts), clones(ts)
    kw = dict(lr=0.1, momentum=momentum, nesterov=nesterov, weight_decay=wd)
    o1, o2 = FusedSGD(p1, **kw), torch.optim.SGD(p2, **kw)
    for s in range(5):
        for a, b, g in zip(p1, p2, tensor_list(seed=10 + s)):
            a.grad, b.grad = g.clone(), g.clone()
        o1.step()
        o2.step()
    for a, b in zip(p1, p2):
        assert (a - b).abs().max().item() < 1e-5
    sd1, sd2 = o1.state_dict(), o2.state_dict()
    assert sd1["state"].keys() == sd2["state"].keys()
    assert sd1["param_groups"][0].keys() == sd2["param_groups"][0].keys()
    for k in sd1["state"]:
        assert sd1["state"][k].keys() == sd2["state"][k].keys() == {"momentum_buffer"}
        assert (sd1["state"][k]["momentum_buffer"] - sd2["state"][k]["momentum_buffer"]).abs().max().item() < 1e-5
    if momentum == 0:
        assert not sd1["state"]


def test_fused_sgd_cpu_tensor_lr_and_skipped_step():
    from pytorch_distributedtraining_amd.optim import FusedSGD
    ts = tensor_list()
    p1, p2 = clones(ts), clones(ts)
    lr = torch.tensor(0.1)
    o1, o2 = FusedSGD(p1, lr=lr, momentum=0.9), torch.optim.SGD(p2, lr=0.1, momentum=0.9)
    for s, rate in enumerate((0.1, 0.05)):
        lr.fill_(rate)
        o2.param_groups[0]["lr"] = rate
        for a, b, g in zip(p1, p2, tensor_list(seed=20 + s)):
            a.grad, b.grad = g.clone(), g.clone()
        o1.step()
        o2.step()
    for a, b in zip(p1, p2):
        assert (a - b).abs().max().item() < 1e-5
    before = [p.detach().clone() for p in p1] + [o1.state[p]["momentum_buffer"].clone() for p in p1]
    o1.step(found_inf=torch.ones(1, dtype=torch.int32))
    after = [p.detach() for p in p1] + [o1.state[p]["momentum_buffer"] for p in p1]
    assert all(torch.equal(a, b) for a, b in zip(before, after))


def test_fused_sgd_rejections_cpu():
    from pytorch_distributedtraining_amd.optim import FusedOptimizer, FusedAdamW, FusedSGD
    assert issubclass(FusedSGD, FusedOptimizer) and issubclass(FusedAdamW, FusedOptimizer)
    p = [nn.Parameter(torch.zeros(4))]
    with pytest.raises(ValueError):
        FusedSGD(p, lr=0.1, momentum=0.9, dampening=0.1)
    with pytest.raises(ValueError):
        FusedSGD(p, lr=0.1, maximize=True)
    with pytest.raises(ValueError):
        FusedSGD(p, lr=0.1, nesterov=True, momentum=0)
    q = nn.Parameter(torch.zeros(4, dtype=torch.bfloat16))
    q.grad = torch.ones(4, dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="FusedSGD keeps fp32 master params"):
        FusedSGD([q], lr=0.1).step()
    e = nn.Embedding(8, 4, sparse=True)
    e(torch.tensor([1, 2])).sum().backward()
    with pytest.raises(RuntimeError, match="sparse"):
        FusedSGD(e.parameters(), lr=0.1).step()


# ------------------------------------------------------------------------------------------- OSS + SDDP, gloo
def _model(seed=0):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Linear(16, 32), nn.Tanh(), nn.Linear(32, 32), nn.Tanh(), nn.Linear(32, 4))


def _data(step, world):
    g = torch.Generator().manual_seed(100 + step)
    return torch.randn(world * 8, 16, generator=g), torch.randn(world * 8, 4, generator=g)


def _shard(x, rank, world):
    n = x.shape[0] // world
    return x[rank * n:(rank + 1) * n]


SGD_KW = dict(lr=1e-2, momentum=0.9, weight_decay=1e-4)


def _reference(world):
    m = _model()
    opt = torch.optim.SGD(m.parameters(), **SGD_KW)
    for s in range(STEPS):
        x, y = _data(s, world)
        opt.zero_grad()
        nn.functional.mse_loss(m(x), y).backward()
        opt.step()
    return {k: v.detach().clone() for k, v in m.state_dict().items()}, opt.state_dict()


def _w_zero_sgd(rank, world):
    from pytorch_distributedtraining_amd.optim import FusedSGD
    from pytorch_distributedtraining_amd.parallel.zero import OSS, ShardedDataParallel
    m = _model()
    opt = OSS(m.parameters(), optim=FusedSGD, **SGD_KW)
    model = ShardedDataParallel(m, opt, reduce_buffer_size=256)
    for s in range(STEPS):
        x, y = _data(s, world)
        model.zero_grad()
        nn.functional.mse_loss(model(_shard(x, rank, world)), _shard(y, rank, world)).backward()
        opt.step()
    opt.consolidate_state_dict(0)
    sd = opt.state_dict() if rank == 0 else None
    return {k: v.detach().clone() for k, v in m.state_dict().items()}, sd


def test_oss_sddp_fused_sgd_matches_single_process_torch_sgd():
    world = 2
    ref, ref_sd = _reference(world)
    outs = run_workers(_w_zero_sgd, world)
    p0, sd = outs[0]
    for k in ref:
        assert torch.equal(p0[k], outs[1][0][k])
        assert torch.allclose(p0[k], ref[k], atol=2e-5), k
    # consolidated state in torch.optim.SGD's layout: a momentum buffer per parameter, no step count
    assert sorted(sd["state"].keys()) == list(range(6))
    for i in range(6):
        assert set(sd["state"][i].keys()) == {"momentum_buffer"}
        assert torch.allclose(sd["state"][i]["momentum_buffer"], ref_sd["state"][i]["momentum_buffer"], atol=2e-5)


def _w_zero_sgd_compute_dtype(rank, world):
    from pytorch_distributedtraining_amd.optim import FusedSGD
    from pytorch_distributedtraining_amd.parallel.zero import OSS, ShardedDataParallel
    m = _model()
    init = {k: v.detach().clone() for k, v in m.state_dict().items()}
    opt = OSS(m.parameters(), optim=FusedSGD, compute_dtype=torch.bfloat16, **SGD_KW)
    assert all(p.dtype == torch.bfloat16 for p in m.parameters())
    assert all(p.dtype == torch.float32 for p in opt.owned_params())
    model = ShardedDataParallel(m, opt)
    for s in range(STEPS):
        x, y = _data(s, world)
        model.zero_grad()
        nn.functional.mse_loss(model(_shard(x, rank, world).bfloat16()).float(), _shard(y, rank, world)).backward()
        opt.step()
    # the module's bf16 parameters are the epilogue's rounding of this rank's fp32 masters
    for p in opt.owned_params():
        assert torch.equal(p._pdt_lp_shard, p.detach().to(torch.bfloat16))
    return init, {k: v.detach().float().clone() for k, v in m.state_dict().items()}


def test_oss_compute_dtype_accepts_fused_sgd():
    outs = run_workers(_w_zero_sgd_compute_dtype, 2)
    init, last = outs[0]
    for k in init:
        assert torch.equal(last[k], outs[1][1][k]), k                 # every rank holds the same bf16 model
        assert not torch.equal(last[k], init[k].bfloat16().float()), k     # ... and it trained


def test_oss_compute_dtype_still_rejects_torch_optimizers():
    from pytorch_distributedtraining_amd.parallel.comm import Comm
    from pytorch_distributedtraining_amd.parallel.zero import OSS
    with pytest.raises(ValueError, match="fused optimizer"):
        OSS(_model().parameters(), optim=torch.optim.SGD, compute_dtype=torch.bfloat16, comm=Comm(), lr=0.1)


def _w_bcast16_frozen_and_skipped(rank, world):
    """broadcast_fp16 payload with a frozen parameter owned by rank 0 and a skipped (found_inf) FIRST step: the
    owner's slice of the all-gather payload must carry current values, never its initial zeros."""
    from pytorch_distributedtraining_amd.optim import FusedSGD
    from pytorch_distributedtraining_amd.parallel.zero import OSS, ShardedDataParallel
    from pytorch_distributedtraining_amd.utils.native import require_runtime
    m = _model()
    names = [n for n, _ in m.named_parameters()]
    # freeze a parameter rank 0 owns (the partition depends on the sizes only)
    owner = list(require_runtime().greedy_partition([p.numel() for p in m.parameters()], world))
    frozen = next(n for n, o in zip(names, owner) if o == 0 and n != "0.weight")
    dict(m.named_parameters())[frozen].requires_grad_(False)
    init = {k: v.detach().clone() for k, v in m.state_dict().items()}
    opt = OSS(m.parameters(), optim=FusedSGD, broadcast_fp16=True, lr=1e-2, momentum=0.9)
    assert list(opt.owner) == owner
    model = ShardedDataParallel(m, opt)
    snaps = []
    for s, inf in enumerate((1.0, 0.0, 0.0)):
        x, y = _data(s, world)
        model.zero_grad()
        nn.functional.mse_loss(model(_shard(x, rank, world)), _shard(y, rank, world)).backward()
        opt.step(found_inf=torch.tensor([inf]))
        snaps.append({k: v.detach().clone() for k, v in m.state_dict().items()})
    return init, snaps, frozen


def test_oss_broadcast_fp16_fused_sgd_frozen_param_and_skipped_step():
    world = 2
    outs = run_workers(_w_bcast16_frozen_and_skipped, world)
    init, frozen = outs[0][0], outs[0][2]
    for r, (_, snaps, _) in enumerate(outs):
        skipped, _, last = snaps
        for k in init:        # the overflowed first step changes nothing (peers: the fp16 payload of it)
            assert torch.allclose(skipped[k], init[k], atol=1e-3, rtol=1e-3), (r, k)
        assert torch.allclose(last[frozen], init[frozen], atol=1e-3, rtol=1e-3), r       # frozen stays put
        assert not torch.allclose(last["0.weight"], init["0.weight"], atol=1e-4)         # others trained
    for k in init:
        assert torch.allclose(outs[0][1][2][k], outs[1][1][2][k], atol=2e-3), k


# ------------------------------------------------------------------------------------------- run configuration
def test_sgd_config_loads_and_trains_on_cpu():
    from pytorch_distributedtraining_amd import train
    from pytorch_distributedtraining_amd.run_config import load_config, optimizer_name
    cfg = load_config(os.path.join(ROOT, "configs", "resnet50_ddp_sgd.yaml"))
    assert cfg.optimizer == {"name": "sgd", "lr": 0.1, "momentum": 0.9, "nesterov": True, "weight_decay": 1e-4}
    assert optimizer_name(cfg.optimizer) == "sgd"
    small = dataclasses.replace(cfg, model="resnet18", gpu=False, precision="fp32", batch_size_per_device=2,
                                image_size=32, num_classes=10, steps=2, warmup=0, log_every=1)
    seen = []
    real = torch.optim.SGD.step

    def spy(self, *a, **kw):
        seen.append((type(self), self.param_groups[0]["momentum"], self.param_groups[0]["nesterov"]))
        return real(self, *a, **kw)
    torch.optim.SGD.step = spy
    try:
        res = train.run(small)
    finally:
        torch.optim.SGD.step = real
    assert res["steps"] == 2 and res["loss"] == res["loss"]
    assert seen == [(torch.optim.SGD, 0.9, True)] * 2


def test_config_without_name_builds_adamw_and_unknown_name_raises(tmp_path):
    from pytorch_distributedtraining_amd import train
    from pytorch_distributedtraining_amd.run_config import load_config, optimizer_name
    cfg = load_config(os.path.join(ROOT, "configs", "resnet18_ddp_cpu.yaml"))
    assert "name" not in cfg.optimizer and optimizer_name(cfg.optimizer) == "adamw"
    assert cfg.optimizer["betas"] == (0.9, 0.99)
    small = dataclasses.replace(cfg, batch_size_per_device=2, image_size=32, num_classes=10, steps=1, warmup=0)
    seen = []
    real = torch.optim.AdamW.step

    def spy(self, *a, **kw):
        seen.append(type(self))
        return real(self, *a, **kw)
    torch.optim.AdamW.step = spy
    try:
        train.run(small)
    finally:
        torch.optim.AdamW.step = real
    assert seen == [torch.optim.AdamW]
    bad = tmp_path / "bad.yaml"
    bad.write_text("model: resnet18\noptimizer: {name: lars, lr: 0.1}\n")
    with pytest.raises(ValueError, match="lars"):
        load_config(str(bad))
    with pytest.raises(ValueError, match="lars"):
        train.run(dataclasses.replace(small, optimizer={"name": "lars", "lr": 0.1}))
