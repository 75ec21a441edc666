"""CPU tests of sliding-window causal attention in ops.attention.self_attention (``window``): its fallback (the rotation
in torch, K/V expanded, SDPA with a band mask), the ``ValueError``s and ``get_model("llama", window=...)``."""
import math

import pytest
import torch

from kungfu_amd.ops.attention import self_attention

H, HKV, DH, S, W = 4, 2, 128, 192, 64


def _f64_band(qkv, base):
    """The definition in float64: the rotation of Q and K (``base``), then softmax over the keys q - W < k <= q."""
    B = qkv.shape[0]
    x = qkv.double().view(B, S, H + 2 * HKV, DH)
    qk, v = x[:, :, :H + HKV], x[:, :, H + HKV:]
    if base is not None:
        ang = torch.arange(S).double()[:, None] * base ** (-torch.arange(DH // 2).double() / (DH // 2))
        (lo, hi), c, s = qk.split(DH // 2, dim=3), ang.cos()[None, :, None], ang.sin()[None, :, None]
        qk = torch.cat((lo * c - hi * s, hi * c + lo * s), dim=3)
    q = qk[:, :, :H].transpose(1, 2)
    k, v = (t.transpose(1, 2).repeat_interleave(H // HKV, dim=1) for t in (qk[:, :, H:], v))
    d = torch.arange(S)[:, None] - torch.arange(S)[None, :]  # query - key
    sc = (q @ k.transpose(-1, -2) / math.sqrt(DH)).masked_fill((d < 0) | (d >= W), float("-inf"))
    return (torch.softmax(sc, dim=-1) @ v).transpose(1, 2).reshape(B, S, H * DH)


@pytest.mark.parametrize("rope", [None, 10000.0])
def test_fallback_matches_f64_band(rope):
    torch.manual_seed(11)
    qkv = torch.randn(2, S, (H + 2 * HKV) * DH, requires_grad=True)
    y, ref = self_attention(qkv, H, causal=True, kv_heads=HKV, rope=rope, window=W), _f64_band(qkv, rope)
    gout = torch.randn_like(y)
    (g,), (gref,) = torch.autograd.grad(y, qkv, gout), torch.autograd.grad(ref, qkv, gout.double())
    # f32 arithmetic (and f32 tables at angles up to 191 rad): 1e-5 of the norm, as the rope fallback's test
    assert (y.double() - ref).norm() <= 1e-5 * ref.norm() and (g.double() - gref.double()).norm() <= 1e-5 * gref.norm()


@pytest.mark.parametrize("window", [S, 1024])
def test_window_at_least_S_is_the_call_without(window):
    torch.manual_seed(12)
    qkv, kw = torch.randn(1, S, (H + 2 * HKV) * DH), dict(causal=True, kv_heads=HKV, rope=10000.0)
    assert torch.equal(self_attention(qkv, H, window=window, **kw), self_attention(qkv, H, **kw))


@pytest.mark.parametrize("kw", [dict(causal=False, window=64), dict(causal=True, window=96), dict(causal=True, window=0),
                                dict(causal=True, window=64, lengths=torch.full((1,), 64, dtype=torch.int32))])
def test_value_errors(kw):
    with pytest.raises(ValueError, match="window"):
        self_attention(torch.randn(1, 128, 3 * 2 * 64), 2, **kw)


def test_llama_window_runs():
    from kungfu_amd.models import get_model
    model = get_model("llama", window=128, vocab=128, d=256, layers=1, heads=2, kv_heads=1, ffn=256)
    assert model.layers[0].window == 128 and torch.isfinite(model(torch.randint(0, 128, (1, 256)))).all()
