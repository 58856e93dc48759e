"""FusedLAMB off the GPU: its torch-op path against the fp64 definition (tests/lamb_ref.py), the segment protocol,
the state layout shared with torch.optim.AdamW, the engines over gloo at world 2, the Trainer and the run
configuration."""
import copy
import dataclasses
import os

import pytest
import torch
import torch.nn as nn

import lamb_ref
import param_ema_ref
from dist_utils import run_workers
from sgd_cases import clones, tensor_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 3


def _grads(n=5, first=10):
    return [tensor_list(seed=first + s) for s in range(n)]


def _run(ps, grad_lists, **kw):
    from pytorch_distributedtraining_amd.optim import FusedLAMB
    opt = FusedLAMB(ps, **kw)
    for grads in grad_lists:
        for p, g in zip(ps, grads):
            p.grad = g.clone().reshape(p.shape)
        opt.step()
    return opt


def _got(ps, opt):
    return ([p.detach() for p in ps], [opt.state[p]["exp_avg"] for p in ps],
            [opt.state[p]["exp_avg_sq"] for p in ps], opt.trust_sums[0])


# ------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("wd,always", [(0.01, False), (0.0, False), (0.0, True)])
def test_cpu_matches_fp64_reference(wd, always):
    ts, grads = tensor_list(), _grads()
    kw = dict(lr=1e-2, weight_decay=wd, always_adapt=always)
    ref, comp = lamb_ref.reference_and_composite(ts, grads, **kw)
    ps = clones(ts)
    opt = _run(ps, grads, **kw)
    lamb_ref.check(_got(ps, opt), ref, comp, f"cpu wd={wd} always={always}")
    if wd == 0 and not always:      # ratio 1: bias-corrected Adam with the eps outside the bias correction
        qs = clones(ts)
        adam = torch.optim.Adam(qs, lr=1e-2, eps=1e-6)
        for gl in grads:
            for q, g in zip(qs, gl):
                q.grad = g.clone()
            adam.step()
        for p, q in zip(ps, qs):
            assert torch.allclose(p, q, atol=1e-5)


def test_zero_norms():
    from pytorch_distributedtraining_amd.optim import FusedLAMB
    g = torch.Generator().manual_seed(3)
    # an all-zero parameter with a non-zero gradient: ||p|| = 0 -> r = 1
    z = [torch.zeros(37)]
    gz = [[torch.randn(37, generator=g)]]
    ref, comp = lamb_ref.reference_and_composite(z, gz, lr=1e-2, weight_decay=0.01)
    ps = clones(z)
    opt = _run(ps, gz, lr=1e-2, weight_decay=0.01)
    assert float(opt.trust_sums[0][0, 0]) == 0.0 and float(opt.trust_sums[0][0, 1]) > 0
    assert torch.isfinite(ps[0]).all() and float(ps[0].detach().abs().max()) > 0
    lamb_ref.check(_got(ps, opt), ref, comp, "zero parameter")
    # a zero gradient at step 1 with wd = 0: u = 0 -> r = 1 (always_adapt, so that the ratio rule is what is tested)
    t = [torch.randn(37, generator=g)]
    g0 = [[torch.zeros(37)]]
    kw = dict(lr=1e-2, weight_decay=0.0, always_adapt=True)
    ref, comp = lamb_ref.reference_and_composite(t, g0, **kw)
    ps = clones(t)
    opt = _run(ps, g0, **kw)
    assert float(opt.trust_sums[0][0, 1]) == 0.0 and float(opt.trust_sums[0][0, 0]) > 0
    assert torch.equal(ps[0].detach(), t[0]) and torch.isfinite(opt.state[ps[0]]["exp_avg_sq"]).all()
    lamb_ref.check(_got(ps, opt), ref, comp, "zero gradient")
    assert isinstance(opt, FusedLAMB)


# ------------------------------------------------------------------------------------------- segments
SPANS = [(16, 100, 0), (128, 1, 1), (160, 333, 2), (496, 16, 3)]      # gaps: [0,16) [116,128) [129,160) [493,496) [512,520)
FLAT_N = 520


def _segmented(n=FLAT_N, spans=SPANS, seed=5):
    from pytorch_distributedtraining_amd.parallel._segments import Segments
    g = torch.Generator().manual_seed(seed)
    flat = nn.Parameter(torch.randn(n, generator=g))
    flat._pdt_segments = Segments(spans, len(spans), None)
    grads = [torch.randn(n, generator=g) for _ in range(STEPS)]
    return flat, grads


def test_segments_match_separate_tensors_and_gaps_keep_their_bits():
    from pytorch_distributedtraining_amd.optim import FusedLAMB
    flat, grads = _segmented()
    init = flat.detach().clone()
    parts = [nn.Parameter(init[s:s + n].clone()) for s, n, _ in SPANS]
    kw = dict(lr=1e-2, weight_decay=0.01, ema_decay=0.9)
    o1, o2 = FusedLAMB([flat], **kw), FusedLAMB(parts, **kw)
    # poison the gaps of the state so that "kept their bits" is not "stayed zero"
    gap = torch.ones(FLAT_N, dtype=torch.bool)
    for s, n, _ in SPANS:
        gap[s:s + n] = False
    for k in range(STEPS):
        flat.grad = grads[k].clone()
        for p, (s, n, _) in zip(parts, SPANS):
            p.grad = grads[k][s:s + n].clone()
        o1.step()
        o2.step()
        if k == 0:
            for key in ("exp_avg", "exp_avg_sq", "ema"):
                o1.state[flat][key][gap] = 7.25
    st = o1.state[flat]
    assert st["exp_avg"].shape == st["exp_avg_sq"].shape == st["ema"].shape == flat.shape      # a flat stays flat
    for p, (s, n, _) in zip(parts, SPANS):
        assert torch.equal(flat.detach()[s:s + n], p.detach())
        for key in ("exp_avg", "exp_avg_sq", "ema"):
            assert torch.equal(st[key][s:s + n], o2.state[p][key]), key
    assert torch.equal(o1.trust_sums[0], o2.trust_sums[0]) and o1.trust_sums[0].shape == (4, 2)
    assert torch.equal(flat.detach()[gap], init[gap])
    for key in ("exp_avg", "exp_avg_sq", "ema"):
        assert bool((st[key][gap] == 7.25).all()), key


def test_segments_reject_bad_spans():
    from pytorch_distributedtraining_amd.parallel._segments import Segments
    with pytest.raises(ValueError):
        Segments([(0, 10, 0), (5, 10, 1)], 2)         # overlap
    with pytest.raises(ValueError):
        Segments([(0, 10, 2)], 2)                     # gid outside
    with pytest.raises(ValueError):
        Segments([(0, 10, 0), (16, 4, 0)], 2)         # one span per tensor


def test_captured_step_with_a_collective_raises(monkeypatch):
    from pytorch_distributedtraining_amd.optim import FusedLAMB

    class _Comm:
        calls = 0

        def all_reduce(self, t, op="sum"):
            self.calls += 1

    flat, grads = _segmented()
    comm = flat._pdt_segments.comm = _Comm()
    opt = FusedLAMB([flat], lr=1e-2)
    flat.grad = grads[0].clone()
    opt.step()
    assert comm.calls == 1                      # ONE all-reduce of the group's sums per step
    before = flat.detach().clone()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="cannot be captured"):
        opt.step()
    assert comm.calls == 1 and torch.equal(flat.detach(), before) and float(opt.state[flat]["step"]) == 1.0
    flat._pdt_segments.comm = None              # no collective in the step: capture is allowed
    opt.step()
    assert float(opt.state[flat]["step"]) == 2.0


# ------------------------------------------------------------------------------------------- state layout
def test_state_layout_is_adamw_and_checkpoints_interchange():
    from pytorch_distributedtraining_amd.optim import FusedLAMB
    ts, grads = tensor_list(), _grads(4)
    kw = dict(lr=1e-2, weight_decay=0.01)
    p1, p2 = clones(ts), clones(ts)
    o1 = _run(p1, grads[:2], **kw)
    adam = torch.optim.AdamW(p2, lr=1e-2)
    for q, g in zip(p2, grads[0]):
        q.grad = g.clone()
    adam.step()
    sd, asd = o1.state_dict(), adam.state_dict()
    assert sd["state"].keys() == asd["state"].keys()
    for k in sd["state"]:
        assert sd["state"][k].keys() == asd["state"][k].keys() == {"step", "exp_avg", "exp_avg_sq"}
        for key in ("exp_avg", "exp_avg_sq"):
            assert sd["state"][k][key].shape == asd["state"][k][key].shape
            assert sd["state"][k][key].dtype == asd["state"][k][key].dtype
        assert float(sd["state"][k]["step"]) == 2.0
    assert sd.keys() == asd.keys() and sd["param_groups"][0]["params"] == asd["param_groups"][0]["params"]
    # LAMB -> torch.optim.AdamW -> LAMB: the state survives, and training continues as if never interrupted
    adam.load_state_dict(copy.deepcopy(sd))
    for k, q in enumerate(p2):
        assert torch.equal(adam.state[q]["exp_avg"], o1.state[p1[k]]["exp_avg"])
        assert float(adam.state[q]["step"]) == 2.0
    back = adam.state_dict()
    p3 = [nn.Parameter(p.detach().clone()) for p in p1]
    o3 = FusedLAMB(p3, **kw)
    o3.load_state_dict(back)
    for gl in grads[2:]:
        for a, b, g in zip(p1, p3, gl):
            a.grad, b.grad = g.clone(), g.clone()
        o1.step()
        o3.step()
    for a, b in zip(p1, p3):
        assert torch.equal(a, b)
        assert torch.equal(o1.state[a]["exp_avg_sq"], o3.state[b]["exp_avg_sq"])
        assert float(o1.state[a]["step"]) == float(o3.state[b]["step"]) == 4.0


def test_skipped_step_and_ema():
    ts, grads = tensor_list(), _grads(3)
    kw = dict(lr=1e-2, weight_decay=0.01, ema_decay=0.9)
    ps = clones(ts)
    from pytorch_distributedtraining_amd.optim import FusedLAMB
    opt = FusedLAMB(ps, **kw)
    track = param_ema_ref.Ema64([p.detach() for p in ps], 0.9)
    for gl in grads:
        for p, g in zip(ps, gl):
            p.grad = g.clone()
        opt.step()
        track.update([p.detach() for p in ps])      # the definition applied to LAMB's new parameters
    track.check([opt.state[p]["ema"] for p in ps], "lamb ema")
    snap = lambda: [t.clone() for p in ps for t in (p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"],
                                                    opt.state[p]["ema"], opt.state[p]["step"])]
    before = snap()
    opt.step(found_inf=torch.ones(1, dtype=torch.int32))
    assert all(torch.equal(a, b) for a, b in zip(before, snap()))
    assert float(opt.state[ps[0]]["step"]) == 3.0


def test_grad_scale_equals_prescaled_gradients():
    ts, grads = tensor_list(), _grads(2)
    p1, p2 = clones(ts), clones(ts)
    from pytorch_distributedtraining_amd.optim import FusedLAMB
    o1, o2 = FusedLAMB(p1, lr=1e-2), FusedLAMB(p2, lr=1e-2)
    for gl in grads:
        for a, b, g in zip(p1, p2, gl):
            a.grad, b.grad = g.clone(), g * 0.25
        o1.step(grad_scale=torch.tensor([0.25]))
        o2.step()
    for a, b in zip(p1, p2):
        assert torch.equal(a, b)


def test_rejections():
    from pytorch_distributedtraining_amd.optim import FusedLAMB, FusedOptimizer
    assert issubclass(FusedLAMB, FusedOptimizer)
    p = [nn.Parameter(torch.zeros(4))]
    for bad in (dict(amsgrad=True), dict(maximize=True), dict(trust_clip=True), dict(max_grad_norm=1.0)):
        with pytest.raises(ValueError, match="FusedLAMB"):
            FusedLAMB(p, lr=0.1, **bad)
    d = FusedLAMB(p).defaults
    assert (d["lr"], d["betas"], d["eps"], d["weight_decay"], d["always_adapt"], d["capturable"], d["ema_decay"]) == \
        (1e-3, (0.9, 0.999), 1e-6, 0.01, False, False, None)


# ------------------------------------------------------------------------------------------- engines, gloo world 2
LAMB_KW = dict(lr=1e-2, weight_decay=0.01)


def _model(seed=0):
    """One large weight (512 elements) and small ones: as ONE FSDP unit at world 2 the shard boundary (element 344 of
    688) cuts the large weight."""
    torch.manual_seed(seed)
    return nn.Sequential(nn.Linear(16, 32), nn.Tanh(), nn.Linear(32, 4))


def _data(step, world):
    g = torch.Generator().manual_seed(100 + step)
    return torch.randn(world * 8, 16, generator=g), torch.randn(world * 8, 4, generator=g)


def _shard(x, rank, world):
    n = x.shape[0] // world
    return x[rank * n:(rank + 1) * n]


def _single(world, steps=STEPS):
    from pytorch_distributedtraining_amd.optim import FusedLAMB
    m = _model()
    opt = FusedLAMB(m.parameters(), **LAMB_KW)
    for s in range(steps):
        x, y = _data(s, world)
        opt.zero_grad()
        nn.functional.mse_loss(m(x), y).backward()
        opt.step()
    return {k: v.detach().clone() for k, v in m.state_dict().items()}, opt.trust_sums[0].clone(), opt.state_dict()


def _fsdp_build():
    from pytorch_distributedtraining_amd.optim import FusedLAMB
    from pytorch_distributedtraining_amd.parallel.fsdp import FullyShardedDataParallel, MixedPrecision
    eng = FullyShardedDataParallel(_model(), mixed_precision=MixedPrecision(torch.float32, torch.float32),
                                   device=torch.device("cpu"))
    return eng, FusedLAMB(eng.flat_parameters(), **LAMB_KW)


def _w_engines(rank, world):
    from pytorch_distributedtraining_amd.optim import FusedLAMB
    from pytorch_distributedtraining_amd.parallel.ddp import DistributedDataParallel
    from pytorch_distributedtraining_amd.parallel.zero import OSS, ShardedDataParallel
    out = {}

    def train(model, opt, zero):
        for s in range(STEPS):
            x, y = _data(s, world)
            zero()
            nn.functional.mse_loss(model(_shard(x, rank, world)), _shard(y, rank, world)).backward()
            opt.step()

    # FSDP: one unit, the large weight cut by the rank boundary
    eng, opt = _fsdp_build()
    units = eng.all_units()
    seg = units[0].flat_param._pdt_segments
    out["fsdp_units"] = len(units)
    out["fsdp_spans"] = list(seg.spans)
    out["fsdp_comm"] = seg.comm is not None
    train(eng, opt, opt.zero_grad)
    out["fsdp_sums"] = opt.trust_sums[0].clone()
    out["fsdp"] = {k: v.detach().clone() for k, v in eng.state_dict().items()}
    full = eng.full_optim_state_dict(opt)
    out["fsdp_full"] = full
    eng2, opt2 = _fsdp_build()
    eng2.load_full_optim_state_dict(opt2, full)
    out["fsdp_restored"] = all(
        torch.equal(opt2.state[b][k], opt.state[a][k]) for a, b in zip(eng.flat_parameters(), eng2.flat_parameters())
        for k in ("exp_avg", "exp_avg_sq")) and all(float(opt2.state[b]["step"]) == STEPS
                                                    for b in eng2.flat_parameters())
    # DDP with flat fp32 masters (the compute-copy layout, fp32 here): segments without a comm
    m = _model()
    ddp = DistributedDataParallel(m, device=torch.device("cpu"), compute_dtype=torch.float32)
    masters = ddp.optimizer_parameters()
    out["ddp_segments"] = [(len(x._pdt_segments.spans), x._pdt_segments.n_logical, x._pdt_segments.comm is None)
                           for x in masters]
    opt = FusedLAMB(masters, **LAMB_KW)
    train(ddp, opt, lambda: (ddp.zero_grad(), opt.zero_grad()))
    out["ddp"] = {k: v.detach().clone() for k, v in ddp.state_dict().items()}
    out["ddp_sums"] = opt.trust_sums[0].clone()
    # DDP + OSS: whole parameters per owner, no segments
    m = _model()
    oss = OSS(m.parameters(), optim=FusedLAMB, **LAMB_KW)
    sddp = ShardedDataParallel(m, oss, reduce_buffer_size=256, reduce_mode="all_reduce")
    out["oss_segments"] = any(hasattr(p, "_pdt_segments") for p in oss.owned_params())
    train(sddp, oss, sddp.zero_grad)
    out["oss"] = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return out


@pytest.fixture(scope="module")
def world2():
    return run_workers(_w_engines, 2), _single(2)


def _strip(sd):
    return {k.replace("module.", ""): v for k, v in sd.items()}


def test_fsdp_cut_weight_matches_single_process_and_all_reduces_norms(world2):
    outs, (ref, ref_sums, _) = world2
    r0, r1 = outs
    assert r0["fsdp_units"] == 1 and r0["fsdp_comm"] and r1["fsdp_comm"]
    # the 512-element weight (gid 0) has a span on BOTH ranks
    assert 0 in {g for _, _, g in r0["fsdp_spans"]} and 0 in {g for _, _, g in r1["fsdp_spans"]}
    assert sum(n for _, n, g in r0["fsdp_spans"] + r1["fsdp_spans"] if g == 0) == 512
    for r in (r0, r1):
        got = _strip(r["fsdp"])
        for k in ref:
            torch.testing.assert_close(got[k], ref[k])
        # after the all-reduce: whole-tensor norms on every rank (local norms would halve the cut weight's)
        torch.testing.assert_close(r["fsdp_sums"], ref_sums)
    assert torch.equal(r0["fsdp_sums"], r1["fsdp_sums"])


def test_ddp_flat_master_matches_single_process(world2):
    outs, (ref, ref_sums, _) = world2
    for r in outs:
        assert r["ddp_segments"] == [(4, 4, True)]
        got = _strip(r["ddp"])
        for k in ref:
            torch.testing.assert_close(got[k], ref[k])
        # one trust ratio per logical tensor, not one for the flat (the parameters' order may differ in the flat)
        torch.testing.assert_close(r["ddp_sums"].sort(0).values, ref_sums.sort(0).values)


def test_ddp_oss_matches_single_process(world2):
    outs, (ref, _, _) = world2
    for r in outs:
        assert not r["oss_segments"]
        for k in ref:
            torch.testing.assert_close(r["oss"][k], ref[k])


def test_fsdp_full_optim_state_round_trip(world2):
    outs, (_, _, ref_sd) = world2
    full = outs[0]["fsdp_full"]
    assert outs[0]["fsdp_restored"] and outs[1]["fsdp_restored"]
    assert sorted(full["state"].keys()) == [0, 1, 2, 3]
    for i in range(4):
        assert set(full["state"][i].keys()) == {"step", "exp_avg", "exp_avg_sq"}
        for k in ("exp_avg", "exp_avg_sq"):
            assert full["state"][i][k].shape == ref_sd["state"][i][k].shape
            torch.testing.assert_close(full["state"][i][k], ref_sd["state"][i][k])


# ------------------------------------------------------------------------------------------- Trainer, configuration
def test_trainer_with_fused_lamb_and_param_ema_on_cpu():
    from pytorch_distributedtraining_amd.optim import FusedLAMB
    from pytorch_distributedtraining_amd.trainer import StokeOptimizer, Trainer
    tr = Trainer(_model(), StokeOptimizer(optimizer=FusedLAMB, optimizer_kwargs=dict(LAMB_KW)),
                 loss=nn.functional.mse_loss, batch_size_per_device=16, gpu=False, verbose=False,
                 param_ema_decay=0.99)
    assert type(tr.optimizer) is FusedLAMB and tr.optimizer.param_groups[0]["ema_decay"] == 0.99
    first = None
    for s in range(STEPS):
        x, y = _data(s, 2)
        loss = tr.loss(tr.model(x), y)
        first = float(loss.detach()) if first is None else first
        tr.backward(loss)
        tr.step()
    ref, ref_sums, _ = _single(2)
    for k, v in tr.model_access.state_dict().items():
        torch.testing.assert_close(v, ref[k])
    torch.testing.assert_close(tr.optimizer.trust_sums[0], ref_sums)
    assert all("ema" in tr.optimizer.state[p] for p in tr.model_access.parameters())
    with tr.averaged_parameters():
        pass


def test_lamb_config_loads_and_trains_on_cpu(tmp_path):
    from pytorch_distributedtraining_amd import train
    from pytorch_distributedtraining_amd.optim import FusedLAMB
    from pytorch_distributedtraining_amd.run_config import OPTIMIZERS, load_config, optimizer_name
    assert "lamb" in OPTIMIZERS and "lars" not in OPTIMIZERS
    cfg = load_config(os.path.join(ROOT, "configs", "gpt2_124m_ddp_lamb.yaml"))
    assert optimizer_name(cfg.optimizer) == "lamb" and cfg.optimizer["weight_decay"] == 0.01
    assert cfg.model == "gpt2-124m" and cfg.distributed == "ddp"
    y = tmp_path / "tiny.yaml"
    y.write_text("model: resnet18\noptimizer: {name: lamb, lr: 1.0e-3, weight_decay: 0.01}\n")
    small = dataclasses.replace(load_config(str(y)), gpu=False, precision="fp32", batch_size_per_device=2,
                                image_size=32, num_classes=10, steps=2, warmup=0, log_every=1)
    seen = []
    real = FusedLAMB.step

    def spy(self, *a, **kw):
        seen.append(type(self))
        return real(self, *a, **kw)
    FusedLAMB.step = spy
    try:
        res = train.run(small)
    finally:
        FusedLAMB.step = real
    assert res["steps"] == 2 and res["loss"] == res["loss"]
    assert seen == [FusedLAMB] * 2
