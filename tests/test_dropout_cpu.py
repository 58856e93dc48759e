"""Mask-free dropout (ops.dropout) on the CPU: Philox known answers, the torch fallback's mask bit for bit against
the numpy reference (tests/dropout_ref.py), autograd, GPT-2 with dropout (eval, seeding, checkpointing) and the
run-config plumbing."""
import os

import numpy as np
import pytest
import torch

import dropout_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = [12345, 0x7123456789ABCDEF, 0x0000000180000000, -1, -0x0123456789ABCDEF, -(1 << 63)]


def _t(v):
    return torch.tensor([v], dtype=torch.int64)


def test_philox_known_answers_reference():
    for c, k, want in R.KAT:
        assert tuple(int(w) for w in R.philox4x32_10(c, k)) == want


def test_philox_known_answers_torch_fallback():
    from pytorch_distributedtraining_amd.ops import dropout as D
    for c, k, want in R.KAT:
        got = D.philox4x32_10(*[_t(v) for v in c], *[_t(v) for v in k])
        assert tuple(int(w) for w in got) == want


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_fallback_mask_equals_reference(key, p):
    from pytorch_distributedtraining_amd.ops import dropout as D
    numel = 8 * 1000 + 3
    thr, scale = D.quantise(p)
    assert (thr, np.float32(scale)) == R.quantise(p)
    got = D.keep_mask(numel, _t(key), thr).numpy()
    assert got.dtype == np.bool_ and got.shape == (numel,)
    assert np.array_equal(got, R.keep_mask(numel, key, p))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_reference_keep_fraction(p):
    """A condition on the reference alone: over 2^20 elements the keep fraction is within 0.005 of
    1 - thr / 65536 (binomial sigma 3e-4 .. 5e-4)."""
    frac = R.keep_mask(1 << 20, 20240229, p).mean()
    assert abs(frac - (1 - R.quantise(p)[0] / 65536)) < 0.005, frac


def test_quantise_bounds():
    from pytorch_distributedtraining_amd.ops import dropout as D
    assert D.quantise(0.0) == (0, 1.0)
    assert D.quantise(0.99999999)[0] == 65535
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError):
            D.quantise(bad)
        with pytest.raises(ValueError):
            D.Dropout(bad)


def test_dropout_autograd_cpu():
    from pytorch_distributedtraining_amd.ops import dropout as D
    torch.manual_seed(0)
    key, p = -77, 0.3
    x = torch.randn(5, 7, 23, requires_grad=True)
    dy = torch.randn(5, 7, 23)
    y = D.dropout(x, p, _t(key))
    y.backward(dy)
    thr, scale = R.quantise(p)
    keep = torch.from_numpy(R.keep_mask(x.numel(), key, p)).view(x.shape)
    assert torch.equal(y, torch.where(keep, x.detach() * float(scale), torch.zeros(())))
    assert torch.equal(x.grad, torch.where(keep, dy * float(scale), torch.zeros(())))
    assert D.dropout(x, p, _t(key), training=False) is x and D.dropout(x, 0.0, _t(key)) is x
    m = D.Dropout(0.3)
    torch.manual_seed(1)
    a = m(x)
    torch.manual_seed(1)
    assert torch.equal(a, m(x)) and not torch.equal(a, m(x))
    assert m.eval()(x) is x


def test_add_norm_dropout_cpu_matches_definition():
    """The composite path (CPU): s = x + drop(r + rb) / s = drop(x + r) with the reference mask."""
    from pytorch_distributedtraining_amd.ops.norms import add_norm
    torch.manual_seed(0)
    N, key, p = 24, 99, 0.25
    x, r, rb = torch.randn(6, N), torch.randn(6, N), torch.randn(N)
    w, b = torch.rand(N) + 0.5, torch.randn(N)
    keep = torch.from_numpy(R.keep_mask(6 * N, key, p)).view(6, N)
    scale = float(R.quantise(p)[1])
    y, s = add_norm(x, r, w, b, 1e-5, r_bias=rb, dropout=(p, _t(key), "residual"))
    want = x + torch.where(keep, (r + rb) * scale, torch.zeros(()))
    assert torch.allclose(s, want) and torch.allclose(y, torch.nn.functional.layer_norm(want, (N,), w, b, 1e-5), atol=1e-5)
    y, s = add_norm(x, r, w, b, 1e-5, dropout=(p, _t(key), "sum"))
    assert torch.allclose(s, torch.where(keep, (x + r) * scale, torch.zeros(())))
    y0, s0 = add_norm(x, r, w, b, 1e-5, r_bias=rb, dropout=(0.0, _t(key), "residual"))
    y1, s1 = add_norm(x, r, w, b, 1e-5, r_bias=rb)
    assert torch.equal(y0, y1) and torch.equal(s0, s1)


def _pair(**kw):
    from pytorch_distributedtraining_amd.models import build_gpt2
    torch.manual_seed(0)
    base = build_gpt2("gpt2-tiny")
    m = build_gpt2("gpt2-tiny", **kw)
    m.load_state_dict(base.state_dict())
    return base, m


def test_gpt2_dropout_eval_and_seeding_cpu():
    base, m = _pair(resid_pdrop=0.1, embd_pdrop=0.1)
    x = torch.randint(0, 512, (2, 33))
    assert torch.equal(m.eval()(x[:, :-1]), base.eval()(x[:, :-1]))
    m.train(), base.train()
    l0 = base(x[:, :-1], labels=x[:, 1:])
    torch.manual_seed(5)
    l1 = m(x[:, :-1], labels=x[:, 1:])
    torch.manual_seed(5)
    l2 = m(x[:, :-1], labels=x[:, 1:])
    torch.manual_seed(6)
    l3 = m(x[:, :-1], labels=x[:, 1:])
    assert l1.item() != l0.item()
    assert l1.item() == l2.item() and l1.item() != l3.item()
    _, only_resid = _pair(resid_pdrop=0.1)
    assert only_resid(x[:, :-1], labels=x[:, 1:]).item() != l0.item()


def test_gpt2_dropout_checkpointing_matches_plain_cpu(monkeypatch):
    from pytorch_distributedtraining_amd.ops import dropout as D
    calls = []

    def fixed(n, device):
        calls.append(n)
        return (torch.arange(n, dtype=torch.int64, device=device) * 0x123456789ABCDEF + 17)

    monkeypatch.setattr(D, "draw_keys", fixed)
    _, plain = _pair(resid_pdrop=0.1, embd_pdrop=0.1)
    _, ckpt = _pair(resid_pdrop=0.1, embd_pdrop=0.1, activation_checkpointing=True)
    x = torch.randint(0, 512, (2, 33))
    for m in (plain, ckpt):
        m(x[:, :-1], labels=x[:, 1:]).backward()
    assert calls == [2 * 2 + 1] * 2          # one draw per forward for all 2 L + 1 sites, none in the recompute
    for (n, a), (_, b) in zip(plain.named_parameters(), ckpt.named_parameters()):
        assert a.grad is not None and torch.equal(a.grad, b.grad), n


def test_gpt2_attn_pdrop_raises():
    from pytorch_distributedtraining_amd.models import build_gpt2
    with pytest.raises(ValueError, match="attention probabilities"):
        build_gpt2("gpt2-tiny", attn_pdrop=0.1)
    with pytest.raises(ValueError):
        build_gpt2("gpt2-tiny", resid_pdrop=1.0)


def test_run_config_dropout_reaches_model():
    from pytorch_distributedtraining_amd.run_config import RunConfig, load_config
    from pytorch_distributedtraining_amd.train import build_model
    model, kind = build_model(RunConfig(model="gpt2-tiny", seq_len=64, dropout=0.2))
    assert kind == "lm" and model.config.embd_pdrop == 0.2 and model.config.resid_pdrop == 0.2
    assert model.h[0].resid_pdrop == 0.2
    assert build_model(RunConfig(model="gpt2-tiny", seq_len=64))[0].config.resid_pdrop == 0.0
    cfg = load_config(os.path.join(ROOT, "configs", "gpt2_124m_ddp_dropout.yaml"))
    assert cfg.dropout == 0.1 and cfg.model == "gpt2-124m"
    base = load_config(os.path.join(ROOT, "configs", "gpt2_124m_ddp.yaml"))
    assert base.dropout == 0.0
    assert {k: v for k, v in cfg.to_dict().items() if k not in ("name", "dropout")} == \
        {k: v for k, v in base.to_dict().items() if k not in ("name", "dropout")}
    with pytest.raises(ValueError):
        build_model(RunConfig(model="llama3-tiny", dropout=0.1))
