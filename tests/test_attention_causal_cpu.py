"""CPU tests of the causal option of ops.attention.self_attention (its fallback) and of the GPT model."""
import math

import pytest
import torch

from kungfu_amd.ops.attention import self_attention


def test_causal_fallback_matches_masked_softmax():
    torch.manual_seed(3)
    B, S, H = 2, 40, 2
    qkv = torch.randn(B, S, 3 * H * 64, requires_grad=True)
    g = torch.randn(B, S, H * 64)
    y = self_attention(qkv, H, causal=True)
    (dx,) = torch.autograd.grad(y, qkv, g)
    x = qkv.detach().double().requires_grad_(True)
    q, k, v = x.view(B, S, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2) / math.sqrt(64.0)).masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), float("-inf"))
    ref = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, S, H * 64)
    (dref,) = torch.autograd.grad(ref, x, g.double())
    assert torch.allclose(y.double(), ref, atol=1e-5, rtol=1e-5)
    assert torch.allclose(dx.double(), dref, atol=1e-5, rtol=1e-5)


def test_causal_with_lengths_is_refused():
    with pytest.raises(ValueError, match="causal attention takes no lengths"):
        self_attention(torch.zeros(2, 64, 3 * 64), 1, 0.0, torch.ones(2, dtype=torch.int32), causal=True)


def test_gpt_runs_on_cpu():
    from kungfu_amd.models import get_model
    from kungfu_amd.models.gpt import lm_loss, synthetic_lm_batch

    torch.manual_seed(0)
    model = get_model("gpt_base", vocab=500, d=64, layers=1, heads=1, ffn=128, max_pos=64)
    loss = lm_loss(model, synthetic_lm_batch(2, 64, 500))
    loss.backward()
    assert math.isfinite(loss.item()) and abs(loss.item() - math.log(500)) < 1.0
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
