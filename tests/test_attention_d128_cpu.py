"""CPU tests of head dim 128 in ops.attention.self_attention (its fallback) and of the gpt_d128 model."""
import math

import pytest
import torch

from kungfu_amd.ops.attention import self_attention


@pytest.mark.parametrize("causal", [False, True])
def test_d128_fallback_matches_f64_composition(causal):
    torch.manual_seed(3)
    B, S, H = 2, 40, 2
    qkv = torch.randn(B, S, 3 * H * 128, requires_grad=True)
    g = torch.randn(B, S, H * 128)
    y = self_attention(qkv, H, causal=causal)
    (dx,) = torch.autograd.grad(y, qkv, g)
    x = qkv.detach().double().requires_grad_(True)
    q, k, v = x.view(B, S, 3, H, 128).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) / math.sqrt(128.0)
    if causal:
        s = s.masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), float("-inf"))
    ref = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, S, H * 128)
    (dref,) = torch.autograd.grad(ref, x, g.double())
    assert torch.allclose(y.double(), ref, atol=1e-5, rtol=1e-5)
    assert torch.allclose(dx.double(), dref, atol=1e-5, rtol=1e-5)


def test_gpt_d128_runs_on_cpu():
    from kungfu_amd.models import get_model
    from kungfu_amd.models.gpt import lm_loss, synthetic_lm_batch

    torch.manual_seed(0)
    model = get_model("gpt_d128", layers=1, vocab=128)
    assert model.layers[0].heads == 8 and model.layers[0].qkv.in_features == 1024
    loss = lm_loss(model, synthetic_lm_batch(2, 64, 128))
    loss.backward()
    assert math.isfinite(loss.item())
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
