"""Stochastic depth (drop path) without a GPU: the per-sample scales against the numpy mask of tests/dropout_ref.py,
the rate ramp, the model argument, checkpoints, the DropPath module and the run configuration."""
import importlib
import os

import numpy as np
import pytest
import torch

import dropout_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = [1, 7, 8, 9, 18]
KEYS = [-0x0123456789ABCDEF, 0x7123456789ABCDEF, 5, -1]
RATES = [0.0, 0.1, 0.5, 0.999]


def _dp():
    # (ops exports the function drop_path under the submodule's name: fetch the module itself)
    return importlib.import_module("pytorch_distributedtraining_amd.ops.drop_path")


def ref_scales(keys, rates, batch):
    """fp32 [sites, batch] from the numpy reference: scale where kept, 0 where dropped."""
    out = np.zeros((len(keys), batch), dtype=np.float32)
    for s, (k, p) in enumerate(zip(keys, rates)):
        out[s] = np.where(R.keep_mask(batch, k, p), R.quantise(p)[1], np.float32(0))
    return out


@pytest.mark.parametrize("batch", BATCHES)
def test_sample_scales_match_numpy_reference(batch):
    DP = _dp()
    keys = [k for k in KEYS for _ in RATES]
    rates = [p for _ in KEYS for p in RATES]
    got = DP.sample_scales(torch.tensor(keys, dtype=torch.int64), DP.site_table(rates), batch)
    want = ref_scales(keys, rates, batch)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(keys), batch)
    assert np.array_equal(got.numpy(), want)
    for s, p in enumerate(rates):
        if p == 0.0:
            assert bool((got[s] == 1.0).all())
    if batch == 18:     # not vacuous: every key drops and keeps samples at 0.5, drops some at 0.999, keeps some at 0.1
        for s, p in enumerate(rates):
            kept = int((got[s] != 0).sum())
            assert (0 < kept < 18) if p == 0.5 else (kept < 18) if p == 0.999 else kept > 0


def test_rate_ramp_is_upstreams():
    from pytorch_distributedtraining_amd.models.swinir import swinir_s_x2
    m = swinir_s_x2(drop_path_rate=0.1)
    assert torch.equal(torch.tensor(m.drop_path_rates(), dtype=torch.float32), torch.linspace(0, 0.1, 24))
    m = swinir_s_x2(depths=[2, 3], num_heads=[6, 6], drop_path_rate=0.3)
    assert torch.equal(torch.tensor(m.drop_path_rates(), dtype=torch.float32), torch.linspace(0, 0.3, 5))
    assert swinir_s_x2().drop_path_rates() == [0.0] * 24


def _fixed_keys(n, device):
    return (torch.arange(n, dtype=torch.int64) * 0x0F1E2D3C4B5A6978 - 0x1234567).to(device)


def _small(**kw):
    from pytorch_distributedtraining_amd.models.swinir import swinir_s_x2
    torch.manual_seed(0)
    return swinir_s_x2(depths=[2, 2], num_heads=[6, 6], **kw)


def test_argument_takes_effect_in_training_only(monkeypatch):
    from pytorch_distributedtraining_amd.ops import dropout as D
    calls = []

    def fixed(n, device):
        calls.append(n)
        return _fixed_keys(n, device)

    monkeypatch.setattr(D, "draw_keys", fixed)
    base, m = _small(), _small(drop_path_rate=0.3)
    m.load_state_dict(base.state_dict())
    x = torch.rand(4, 3, 16, 24)
    base.train(), m.train()
    y0, y1 = base(x), m(x)
    assert calls == [2 * 4]                       # one draw for all sites of the forward, none at rate 0
    assert not torch.equal(y0, y1) and bool(torch.isfinite(y1).all())
    assert torch.equal(m(x), y1)                  # the same keys give the same samples
    base.eval(), m.eval()
    with torch.no_grad():
        assert torch.equal(base(x), m(x))
    assert calls == [8, 8]


def test_block_on_its_own_draws_two_keys(monkeypatch):
    from pytorch_distributedtraining_amd.models.swinir import SwinTransformerBlock
    from pytorch_distributedtraining_amd.ops import dropout as D
    calls = []

    def fixed(n, device):
        calls.append(n)
        return _fixed_keys(n, device) + 3

    monkeypatch.setattr(D, "draw_keys", fixed)
    torch.manual_seed(0)
    blk = SwinTransformerBlock(60, (16, 16), 6, window_size=8, shift_size=4, drop_path=0.5).train()
    x = torch.randn(6, 256, 60)
    y = blk(x, (16, 16))
    assert calls == [2]
    keep_a = R.keep_mask(6, int(_fixed_keys(2, "cpu")[0]) + 3, 0.5)
    keep_m = R.keep_mask(6, int(_fixed_keys(2, "cpu")[1]) + 3, 0.5)
    both = torch.from_numpy(~keep_a & ~keep_m)
    assert 0 < int(both.sum()) < 6                # some sample loses both branches: the block is the identity there
    assert torch.equal(y[both], x[both]) and not torch.equal(y[~both], x[~both])
    blk.eval()
    blk(x, (16, 16))
    assert calls == [2]


def test_parameters_and_checkpoints_unchanged(tmp_path):
    from pytorch_distributedtraining_amd.models.swinir import swinir_s_x2
    base, m = swinir_s_x2(), swinir_s_x2(drop_path_rate=0.1)
    assert sum(p.numel() for p in m.parameters()) == 910152
    assert list(m.state_dict().keys()) == list(base.state_dict().keys())
    path = tmp_path / "ckpt.pth"
    torch.save({"params": base.state_dict()}, path)
    m.load_state_dict(torch.load(path)["params"], strict=True)
    for (n, a), (_, b) in zip(base.state_dict().items(), m.state_dict().items()):
        assert torch.equal(a, b), n


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float64])
def test_drop_path_module(dt, monkeypatch):
    from pytorch_distributedtraining_amd.ops import DropPath
    from pytorch_distributedtraining_amd.ops import dropout as D
    key = 0x7123456789ABCDEF
    monkeypatch.setattr(D, "draw_keys", lambda n, device: torch.full((n,), key, dtype=torch.int64, device=device))
    m = DropPath(0.5).train()
    B = 9
    keep = torch.from_numpy(R.keep_mask(B, key, 0.5))
    assert 0 < int(keep.sum()) < B
    x = torch.randn(B, 5, 7).to(dt)
    x[~keep] = float("nan")                       # a dropped sample's values never reach the output ...
    x.requires_grad_()
    y = m(x)
    scale = float(R.quantise(0.5)[1])
    xd = x.detach()
    want = (xd.float() * scale).to(dt) if dt != torch.float64 else xd * scale
    assert torch.equal(y[keep], want[keep])
    assert torch.equal(y[~keep], torch.zeros_like(y[~keep]))
    dy = torch.randn(B, 5, 7).to(dt)
    dy[~keep] = float("nan")                      # ... nor do a dropped sample's gradients reach the input's
    y.backward(dy)
    wantg = (dy.float() * scale).to(dt) if dt != torch.float64 else dy * scale
    assert torch.equal(x.grad[keep], wantg[keep])
    assert torch.equal(x.grad[~keep], torch.zeros_like(x.grad[~keep]))
    assert m.eval()(x) is x
    assert DropPath(0.0).train()(x) is x
    with pytest.raises(ValueError):
        DropPath(1.0)


def test_drop_path_add_cpu():
    from pytorch_distributedtraining_amd.ops import drop_path_add
    sc = torch.tensor([1.25, 0.0, 1.25])
    x = torch.randn(3, 4, 5, requires_grad=True)
    r = torch.randn(3, 4, 5)
    r[1] = float("inf")
    r.requires_grad_()
    y = drop_path_add(x, r, sc)
    assert torch.equal(y[1], x.detach()[1]) and torch.equal(y[0], x.detach()[0] + r.detach()[0] * 1.25)
    dy = torch.randn_like(y)
    y.backward(dy)
    assert torch.equal(x.grad, dy)
    assert torch.equal(r.grad[1], torch.zeros(4, 5)) and torch.equal(r.grad[2], dy[2] * 1.25)


def test_cli_and_config_reach_the_model(monkeypatch):
    from pytorch_distributedtraining_amd import train
    from pytorch_distributedtraining_amd.run_config import RunConfig, load_config
    model, kind = train.build_model(RunConfig(model="swinir-s-x2", drop_path=0.2))
    assert kind == "sr" and model.drop_path_rate == 0.2
    assert torch.equal(torch.tensor(model.drop_path_rates(), dtype=torch.float32), torch.linspace(0, 0.2, 24))
    assert train.build_model(RunConfig(model="swinir-s-x2"))[0].drop_path_rate == 0.0
    cfg = load_config(os.path.join(ROOT, "configs", "swinir_stoke_droppath.yaml"))
    base = load_config(os.path.join(ROOT, "configs", "swinir_stoke.yaml"))
    assert cfg.drop_path == 0.1 and base.drop_path == 0.0
    assert {k: v for k, v in cfg.to_dict().items() if k not in ("name", "drop_path")} == \
        {k: v for k, v in base.to_dict().items() if k not in ("name", "drop_path")}
    assert train.build_model(cfg)[0].drop_path_rate == 0.1
    with pytest.raises(ValueError, match="drop_path"):
        train.build_model(RunConfig(model="gpt2-tiny", seq_len=64, drop_path=0.1))
    # the command line: --drop-path overrides the file
    seen = {}

    def fake_run(c):
        seen["cfg"] = c
        return {}

    monkeypatch.setattr(train, "run", fake_run)
    train.main(["--config", os.path.join(ROOT, "configs", "swinir_stoke.yaml"), "--drop-path", "0.25"])
    assert seen["cfg"].drop_path == 0.25 and train.build_model(seen["cfg"])[0].drop_path_rate == 0.25
