"""Inputs and float64 expectations shared by the streaming-attention tests (CPU and GPU).

The known-answer case: every key row of a (sequence, head) is the same vector, so each query's
scores are all equal, its probabilities are exactly 1/S (S a power of two) and the output is the
column mean of V.  Q, K, V are small integers (exact in bf16), V's 64-key blocks carry different
constant offsets (a skipped or doubled key block changes the sums)."""
import torch

from kungfu_amd.utils.numerics import integer_data

B, H, DH = 2, 3, 64
# one per 64-key block, S <= 512; they do not cancel, so the column sums leave bf16's exact integers (256)
V_BLOCK_OFFSETS = (3, -2, 5, 4, -1, 6, 2, 7)


def known_answer(S: int):
    """(qkv [B, S, 3*H*64] f32 of integers, column sums of V [B, H, 64] f64, score*scale [B, H, S] f64)."""
    q = integer_data((B, S, H, DH), "dense", seed=7)
    k = integer_data((B, 1, H, DH), "sparse", seed=8).expand(B, S, H, DH)
    off = torch.tensor(V_BLOCK_OFFSETS[:S // 64], dtype=torch.float32).repeat_interleave(64).view(1, S, 1, 1)
    v = integer_data((B, S, H, DH), "dense", seed=9) + off
    qkv = torch.stack([q, k, v], dim=2).reshape(B, S, 3 * H * DH).contiguous()
    vsum = v.double().sum(1)                                                 # [B, H, 64]
    score = (q.double() * k.double()).sum(-1).permute(0, 2, 1) / 8.0         # [B, H, S]
    return qkv, vsum, score
