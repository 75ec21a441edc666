"""CPU test of self_attention's torch composition for padded batches (ops.attention._lengths_fallback)."""
import pytest
import torch

from kungfu_amd.ops.attention import self_attention

B, H = 2, 3


@pytest.mark.parametrize("S,lengths", [(128, (128, 1)), (128, (65, 64)), (128, (0, 100)), (192, (192, 63)),
                                       (192, (129, 17)), (512, (300, 449)), (512, (512, 1)), (64, (64, 3))])
def test_lengths_fallback_matches_float64(S, lengths):
    """f32 on the CPU against a float64 composition written per sequence (a plain softmax over its first L keys):
    1e-5 relative L2 (f32 rounding over at most 512 keys), padded rows of out and dqkv exactly zero, L = 0 finite."""
    torch.manual_seed(3)
    qkv = torch.randn(B, S, 3 * H * 64, requires_grad=True)
    gout = torch.randn(B, S, H * 64)
    out = self_attention(qkv, H, 0.0, torch.tensor(lengths, dtype=torch.int32))
    out.backward(gout)
    x = qkv.detach().double().requires_grad_(True)
    ref = torch.zeros(B, S, H * 64, dtype=torch.float64)
    rows = []
    for b, L in enumerate(lengths):
        q, k, v = x[b, :L].view(L, 3, H, 64).permute(1, 2, 0, 3)
        rows.append((torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1) @ v).transpose(0, 1).reshape(L, H * 64))
        rows.append(ref[b, L:])
    ref = torch.cat(rows).view(B, S, H * 64)
    ref.backward(gout.double())
    for got, want in ((out.detach(), ref.detach()), (qkv.grad, x.grad)):
        assert torch.isfinite(got).all()
        assert ((got.double() - want).norm() / want.norm()).item() < 1e-5
        for b, L in enumerate(lengths):
            assert not got[b, L:].any() and not want[b, L:].any()
