"""Label smoothing and z-loss without a GPU: the op's torch fallback against the fp64 reference of tests/ce_ref.py,
argument validation, the ``nn.CrossEntropyLoss`` drop-in, and the plumbing through the model configs, ``RunConfig``,
``train.build_model`` / ``train.loss_fn`` and a two-step ResNet-18 run."""
import dataclasses
import json
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import ce_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("dt", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("eps,z", [(0.1, 0.0), (0.0, 1e-2), (0.1, 1e-2)])
def test_fallback_matches_fp64_reference(dt, eps, z):
    """CPU logits, and fp16 logits on any device, take the torch composite: F.cross_entropy(label_smoothing=) plus
    z * logsumexp^2 masked and reduced the same way -- the definition the kernels implement."""
    from pytorch_distributedtraining_amd.ops import cross_entropy
    x0, t = R.make_case(17, 1000, dt, "cpu")
    grow = torch.rand(17, generator=torch.Generator().manual_seed(5)) + 0.5
    # the fallback computes in fp32 from the same values (1e-4, the fp32 kernels' bound); an fp16 leaf receives its
    # gradient rounded to fp16, 2^-11 per element: norm-wise below 2^-10 with the fp32 error on top
    gtol = 1e-4 if dt == torch.float32 else 2.0 ** -10
    for reduction, up in (("mean", None), ("sum", None), ("none", grow)):
        want, gwant = R.assert_not_vacuous(x0, t, eps, z, reduction, gtol, up)
        x = x0.clone().requires_grad_()
        loss = cross_entropy(x, t, reduction=reduction, label_smoothing=eps, z_loss=z)
        loss.backward(up)
        assert loss.dtype == torch.float32 and loss.shape == want.shape
        assert R.loss_close(loss, want)
        assert R.rel_err(x.grad, gwant) < gtol
        assert float(x.grad[3].abs().max()) == 0.0
        if reduction == "none":
            assert float(loss.detach()[3]) == 0.0


def test_validation():
    from pytorch_distributedtraining_amd import ops
    from pytorch_distributedtraining_amd.models.gpt2 import GPT2Config
    from pytorch_distributedtraining_amd.models.llama import LlamaConfig
    x, t = torch.randn(4, 10), torch.randint(0, 10, (4,))
    for kw in (dict(label_smoothing=1.0), dict(label_smoothing=1.5), dict(label_smoothing=-0.1), dict(z_loss=-1e-4)):
        with pytest.raises(ValueError):
            ops.cross_entropy(x, t, **kw)
        with pytest.raises(ValueError):
            ops.CrossEntropyLoss(**kw)
        with pytest.raises(ValueError):
            GPT2Config(**kw)
        with pytest.raises(ValueError):
            LlamaConfig(**kw)
    with pytest.raises(ValueError):
        ops.CrossEntropyLoss(weight=torch.ones(10))
    assert (GPT2Config().label_smoothing, GPT2Config().z_loss) == (0.0, 0.0)
    assert (LlamaConfig().label_smoothing, LlamaConfig().z_loss) == (0.0, 0.0)


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_module_is_an_nn_cross_entropy_loss_drop_in(reduction):
    from pytorch_distributedtraining_amd import ops
    assert "CrossEntropyLoss" in ops.__all__
    x, t = R.make_case(9, 40, torch.float32, "cpu", ignore_row=2)
    t[2] = 7
    t[5] = -1
    ours = ops.CrossEntropyLoss(ignore_index=-1, reduction=reduction, label_smoothing=0.1)
    theirs = nn.CrossEntropyLoss(ignore_index=-1, reduction=reduction, label_smoothing=0.1)
    a, b = x.clone().requires_grad_(), x.clone().requires_grad_()
    la, lb = ours(a, t), theirs(b, t)
    assert torch.equal(la, lb)
    la.sum().backward()
    lb.sum().backward()
    assert torch.equal(a.grad, b.grad)
    assert not list(ours.state_dict())                   # no buffers or parameters: nothing joins a checkpoint
    # 3-d logits [B, S, V] with [B, S] targets, as the LM heads call the op
    z3 = ops.CrossEntropyLoss(reduction=reduction, label_smoothing=0.1, z_loss=1e-2)
    x3, t3 = x.reshape(3, 3, 40), t.clamp_min(0).reshape(3, 3)
    want, _ = R.ce_ref(x, t.clamp_min(0), 0.1, 1e-2, reduction)
    assert R.loss_close(z3(x3, t3).reshape(want.shape), want)


def test_run_config_keys_cli_and_shipped_configs(tmp_path):
    from pytorch_distributedtraining_amd.run_config import RunConfig, load_config
    assert (RunConfig().label_smoothing, RunConfig().z_loss) == (0.0, 0.0)
    p = tmp_path / "c.yaml"
    p.write_text("model: gpt2-tiny\nlabel_smoothing: 0.05\nz_loss: 1.0e-4\n")
    cfg = load_config(str(p))
    assert (cfg.label_smoothing, cfg.z_loss) == (0.05, 1e-4)
    assert load_config(str(p), label_smoothing=0.2, z_loss=None).label_smoothing == 0.2       # the CLI's overrides
    sm = load_config(os.path.join(ROOT, "configs", "resnet50_ddp_sgd_smooth.yaml"))
    base = load_config(os.path.join(ROOT, "configs", "resnet50_ddp_sgd.yaml"))
    assert sm.label_smoothing == 0.1 and sm.z_loss == 0.0
    assert dataclasses.replace(sm, name=base.name, label_smoothing=0.0) == base              # the SGD recipe otherwise
    zl = load_config(os.path.join(ROOT, "configs", "gpt2_124m_ddp_zloss.yaml"))
    base = load_config(os.path.join(ROOT, "configs", "gpt2_124m_ddp.yaml"))
    assert zl.z_loss == 1e-4 and zl.label_smoothing == 0.0
    assert dataclasses.replace(zl, name=base.name, z_loss=0.0) == base


def test_train_cli_flags(tmp_path, monkeypatch):
    from pytorch_distributedtraining_amd import train
    seen = {}
    monkeypatch.setattr(train, "run", lambda cfg: seen.update(cfg=cfg) or {"ok": True})
    p = tmp_path / "c.json"
    p.write_text(json.dumps({"model": "resnet18", "gpu": False}))
    assert train.main(["--config", str(p), "--label-smoothing", "0.1", "--z-loss", "1e-4"]) == 0
    assert (seen["cfg"].label_smoothing, seen["cfg"].z_loss) == (0.1, 1e-4)


def test_loss_fn_and_build_model():
    from pytorch_distributedtraining_amd import train
    from pytorch_distributedtraining_amd.run_config import RunConfig
    out = torch.randn(6, 10, generator=torch.Generator().manual_seed(0)) * 3
    tgt = torch.tensor([0, 9, 3, 3, 1, 7])
    smooth = train.loss_fn(RunConfig(model="resnet18", label_smoothing=0.1), "cls")(out, tgt)
    assert torch.allclose(smooth, F.cross_entropy(out, tgt, label_smoothing=0.1), rtol=1e-6, atol=1e-6)
    plain = train.loss_fn(RunConfig(model="resnet18"), "cls")(out, tgt)
    assert torch.equal(plain, F.cross_entropy(out, tgt)) and not torch.allclose(plain, smooth, rtol=1e-3)
    both = train.loss_fn(RunConfig(model="srnet", loss="ce", label_smoothing=0.1, z_loss=1e-2), "sr")
    want, _ = R.ce_ref(out, tgt, 0.1, 1e-2)
    assert R.loss_close(both(out, tgt), want)
    for model in ("swinir-s-x2", "srnet"):
        with pytest.raises(ValueError):
            train.build_model(RunConfig(model=model, label_smoothing=0.1))
        with pytest.raises(ValueError):
            train.build_model(RunConfig(model=model, z_loss=1e-4))
    for model in ("gpt2-tiny", "llama3-tiny"):
        m, kind = train.build_model(RunConfig(model=model, seq_len=64, label_smoothing=0.1, z_loss=1e-4))
        assert kind == "lm" and (m.config.label_smoothing, m.config.z_loss) == (0.1, 1e-4)
        m, _ = train.build_model(RunConfig(model=model, seq_len=64))
        assert (m.config.label_smoothing, m.config.z_loss) == (0.0, 0.0)


def test_lm_heads_regularise_in_training_only():
    """GPT-2-tiny and Llama-tiny on the CPU: the training loss is the regularised one, eval() returns plain
    cross-entropy, and no state-dict key is added."""
    from pytorch_distributedtraining_amd.models import build_gpt2
    from pytorch_distributedtraining_amd.models.llama import build_llama
    for build, name, vocab in ((build_gpt2, "gpt2-tiny", 512), (build_llama, "llama3-tiny", 1024)):
        torch.manual_seed(0)
        base = build(name)
        m = build(name, label_smoothing=0.1, z_loss=1e-2)
        assert list(m.state_dict()) == list(base.state_dict())
        m.load_state_dict(base.state_dict())
        x = torch.randint(0, vocab, (2, 33))
        ids, labels = x[:, :-1], x[:, 1:]
        with torch.no_grad():
            logits = base.eval()(ids).float()
            logits = logits.reshape(-1, logits.shape[-1])
            want, _ = R.ce_ref(logits, labels.reshape(-1), 0.1, 1e-2)
            plain, _ = R.ce_ref(logits, labels.reshape(-1))
            assert abs(want.item() - plain.item()) >= 10 * R.LOSS_TOL * max(1.0, abs(want.item()))
            assert R.loss_close(m.train()(ids, labels), want)
            assert R.loss_close(m.eval()(ids, labels), plain)
            assert R.loss_close(base.train()(ids, labels), plain)


def test_two_step_resnet18_run_with_label_smoothing():
    from pytorch_distributedtraining_amd import train
    from pytorch_distributedtraining_amd.run_config import load_config
    kw = dict(steps=2, warmup=0, image_size=32, batch_size_per_device=2, log_every=1)
    path = os.path.join(ROOT, "configs", "resnet18_ddp_cpu.yaml")
    plain = train.run(dataclasses.replace(load_config(path), **kw))
    smooth = train.run(dataclasses.replace(load_config(path), label_smoothing=0.1, **kw))
    assert smooth["loss"] == smooth["loss"] and abs(smooth["loss"]) != float("inf")
    assert smooth["loss"] != plain["loss"]
