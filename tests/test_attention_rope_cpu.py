"""CPU tests of rotary position embeddings in ops.attention.self_attention (``rope``: its fallback, the rotation in
torch around the call without ``rope``), of ``GPTLM(rope=...)`` and of the gpt_rope model."""
import math

import pytest
import torch

from kungfu_amd.ops.attention import self_attention


def _f64_definition(qkv, H, Hkv, dh, base, causal, lengths):
    """The definition in float64: the rotation of every Q and K head, then softmax(Q K^T / sqrt(dh)) V."""
    B, S, _ = qkv.shape
    x = qkv.double().view(B, S, H + 2 * Hkv, dh)
    ang = torch.arange(S).double()[:, None] * base ** (-torch.arange(dh // 2).double() / (dh // 2))
    c, s = ang.cos()[None, :, None], ang.sin()[None, :, None]
    lo, hi = x[:, :, :H + Hkv].split(dh // 2, dim=3)
    qk = torch.cat((lo * c - hi * s, hi * c + lo * s), dim=3)
    q = qk[:, :, :H].transpose(1, 2)
    k, v = (t.transpose(1, 2).repeat_interleave(H // Hkv, dim=1) for t in (qk[:, :, H:], x[:, :, H + Hkv:]))
    sc = q @ k.transpose(-1, -2) / math.sqrt(dh)
    if causal:
        sc = sc.masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), float("-inf"))
    valid = torch.arange(S).view(1, S) < (torch.full((B,), S) if lengths is None else lengths).view(B, 1)
    out = torch.softmax(sc.masked_fill(~valid.view(B, 1, 1, S), float("-inf")), dim=-1) @ v
    return (out.transpose(1, 2) * valid.view(B, S, 1, 1)).reshape(B, S, H * dh)


@pytest.mark.parametrize("dh,Hkv,causal,lengths", [(64, None, False, None), (64, 2, True, None), (128, None, True, None),
                                                   (128, 1, False, None), (64, None, False, (40, 17))])
def test_fallback_matches_f64_definition(dh, Hkv, causal, lengths):
    torch.manual_seed(7)
    H, B, S, kv = 4, 2, 40, 4 if Hkv is None else Hkv
    qkv = torch.randn(B, S, (H + 2 * kv) * dh, requires_grad=True)
    L = None if lengths is None else torch.tensor(lengths, dtype=torch.int32)
    y = self_attention(qkv, H, 0.0, L, causal, Hkv, rope=10000.0)
    ref = _f64_definition(qkv, H, kv, dh, 10000.0, causal, L)
    gout = torch.randn_like(y)
    (g,), (gref,) = torch.autograd.grad(y, qkv, gout), torch.autograd.grad(ref, qkv, gout.double())
    # f32 arithmetic and f32 tables at angles up to 39 rad: 1e-5 of the norm, as the grouped-query fallback's test
    assert y.shape == ref.shape and (y.double() - ref).norm() <= 1e-5 * ref.norm()
    assert (g.double() - gref.double()).norm() <= 1e-5 * gref.norm()


def test_fallback_gradcheck():
    qkv = torch.randn(1, 3, (2 + 2) * 4, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda x: self_attention(x, 2, causal=True, kv_heads=1, rope=100.0), (qkv,))


@pytest.mark.parametrize("rope", [0.0, -1.0, float("inf"), float("nan"), "10000", True])
def test_value_errors(rope):
    with pytest.raises(ValueError, match="rope"):
        self_attention(torch.randn(1, 8, 3 * 2 * 8), 2, rope=rope)


def test_gpt_rope_has_no_position_table():
    from kungfu_amd.models import get_model
    from kungfu_amd.models.bert import BertLayer
    from kungfu_amd.models.gpt import GPTLM, lm_loss, synthetic_lm_batch

    assert not any(k.startswith("pos") for k in GPTLM(64, 32, 1, 2, 64, rope=10000.0).state_dict())
    model = get_model("gpt_rope", vocab=128, layers=1)
    assert model.pos is None and model.layers[0].rope == 10000.0 and model.layers[0].kv_heads == 2
    lm_loss(model, synthetic_lm_batch(2, 64, 128)).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    names = {m + t for m in ("qkv", "out", "ln1", "fc1", "fc2", "ln2") for t in (".weight", ".bias")}
    assert set(BertLayer(64, 2, 64).state_dict()) == names == set(BertLayer(64, 2, 64, rope=10000.0).state_dict())
    assert set(get_model("gpt_gqa", vocab=128, layers=1).state_dict()) == set(model.state_dict()) | {"pos.weight"}
