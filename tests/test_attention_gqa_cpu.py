"""CPU tests of grouped-query attention in ops.attention.self_attention (``kv_heads``: its fallback), of
``BertLayer(kv_heads=...)`` and of the gpt_gqa model."""
import math

import pytest
import torch

from kungfu_amd.ops.attention import self_attention


def _f64_composition(qkv, g, H, Hkv, dh, causal):
    """(out, dqkv) in float64 from the [B, S, (H + 2*Hkv)*dh] layout: K/V expanded, autograd sums the group."""
    B, S, _ = qkv.shape
    x = qkv.detach().double().requires_grad_(True)
    q, k, v = x.split((H * dh, Hkv * dh, Hkv * dh), dim=2)
    q = q.view(B, S, H, dh).transpose(1, 2)
    k, v = (t.view(B, S, Hkv, dh).transpose(1, 2).repeat_interleave(H // Hkv, dim=1) for t in (k, v))
    s = q @ k.transpose(-1, -2) / math.sqrt(dh)
    if causal:
        s = s.masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), float("-inf"))
    out = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, S, H * dh)
    return out.detach(), torch.autograd.grad(out, x, g.double())[0]


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("B,S,H,Hkv,dh", [(2, 40, 4, 2, 16), (1, 64, 4, 1, 128)])
def test_gqa_fallback_matches_f64_composition(B, S, H, Hkv, dh, causal):
    torch.manual_seed(3)
    qkv = torch.randn(B, S, (H + 2 * Hkv) * dh, requires_grad=True)
    g = torch.randn(B, S, H * dh)
    y = self_attention(qkv, H, causal=causal, kv_heads=Hkv)
    (dx,) = torch.autograd.grad(y, qkv, g)
    ref, dref = _f64_composition(qkv, g, H, Hkv, dh, causal)
    assert y.shape == (B, S, H * dh) and dx.shape == qkv.shape
    assert (y.double() - ref).norm() <= 1e-5 * ref.norm()
    assert (dx.double() - dref).norm() <= 1e-5 * dref.norm()


def test_kv_heads_equal_to_heads_is_the_plain_call():
    torch.manual_seed(4)
    qkv = torch.randn(2, 24, 3 * 2 * 16)
    for causal in (False, True):
        assert torch.equal(self_attention(qkv, 2, causal=causal, kv_heads=2), self_attention(qkv, 2, causal=causal))


@pytest.mark.parametrize("kw", [dict(kv_heads=3), dict(kv_heads=0), dict(kv_heads=2, lengths=True)])
def test_value_errors(kw):
    qkv = torch.randn(2, 16, (4 + 2 * max(kw["kv_heads"], 1)) * 8)
    if kw.get("lengths"):
        kw["lengths"] = torch.full((2,), 8, dtype=torch.int32)
    with pytest.raises(ValueError):
        self_attention(qkv, 4, **kw)


def test_gpt_gqa_runs_on_cpu():
    from kungfu_amd.models import get_model
    from kungfu_amd.models.gpt import lm_loss, synthetic_lm_batch

    torch.manual_seed(0)
    model = get_model("gpt_gqa", vocab=128, layers=1, max_pos=64)
    assert model.layers[0].heads == 8 and model.layers[0].kv_heads == 2
    assert model.layers[0].qkv.weight.shape == ((8 + 4) * 128, 1024)
    loss = lm_loss(model, synthetic_lm_batch(2, 64, 128))
    loss.backward()
    assert math.isfinite(loss.item())
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())


def test_default_bert_layer_is_unchanged():
    from kungfu_amd.models.bert import BertLayer

    shapes = {k: tuple(v.shape) for k, v in BertLayer(256, 4, 512).state_dict().items()}
    want = {"qkv": (768, 256), "out": (256, 256), "fc1": (512, 256), "fc2": (256, 512)}
    expect = {}
    for name, (o, i) in want.items():
        expect[name + ".weight"], expect[name + ".bias"] = (o, i), (o,)
    for ln in ("ln1", "ln2"):
        expect[ln + ".weight"], expect[ln + ".bias"] = (256,), (256,)
    assert shapes == expect
