"""CPU checks behind the streaming-attention tests: the known-answer case's expectation is exact
as claimed (float64 torch), and the KUNGFU_ATTN_LONG knob is registered and documented."""
import os

import pytest
import torch

from attention_long_cases import B, H, V_BLOCK_OFFSETS, known_answer
from conftest import ROOT


@pytest.mark.parametrize("S", [256, 512])
def test_known_answer_is_exact(S):
    qkv, vsum, score = known_answer(S)
    x = qkv.view(B, S, 3, H, 64)
    assert torch.equal(x.bfloat16().float(), x), "inputs exact in bf16"
    q, k, v = (x[:, :, t].double() for t in range(3))
    assert torch.equal(k, k[:, :1].expand_as(k)), "all key rows equal"
    # every score of a query is the same exact number: integer dot products far below 2^24, times 1/8
    s = torch.einsum("bqhd,bkhd->bhqk", q, k)
    assert torch.equal(s, s[..., :1].expand_as(s)) and s.abs().max() < 2 ** 24
    assert torch.equal(s[..., 0] / 8.0, score) and torch.equal(score.float().double(), score)
    # so softmax is exactly 1/S (S a power of two) and O = colsum(V) / S
    P = torch.softmax(s / 8.0, dim=-1)
    assert torch.equal(P, torch.full_like(P, 1.0 / S))
    o = torch.einsum("bhqk,bkhd->bqhd", P, v)
    assert torch.equal(o, (vsum / S).view(B, 1, H, 64).expand_as(o))
    # the f32 sum is exact in any order (integers, every partial sum below 2^24), and so is the division
    assert torch.equal(vsum, vsum.round()) and v.abs().sum(1).max() < 2 ** 24
    assert torch.equal((vsum / S).float().double(), vsum / S)
    # rounding to bf16 commutes with the power-of-two scale: RNE(colsum / S) * S == RNE(colsum)
    assert torch.equal((vsum / S).float().bfloat16().double() * S, vsum.float().bfloat16().double())
    # the rounding is exercised (sums that are not bf16 values) ...
    assert (vsum.float().bfloat16().double() != vsum).float().mean() > 0.25
    # ... and a skipped or doubled 64-key block changes the rounded answer of every column
    for j in range(S // 64):
        blk = v[:, 64 * j:64 * (j + 1)].sum(1)
        for wrong in (vsum - blk, vsum + blk):
            changed = (wrong / S).float().bfloat16() != (vsum / S).float().bfloat16()
            assert changed.float().mean() > 0.9, (j, changed.float().mean())
    assert len(set(V_BLOCK_OFFSETS)) == len(V_BLOCK_OFFSETS)


def test_attn_long_knob_registered_and_documented():
    from kungfu_amd import knobs

    k = knobs.KNOBS["KUNGFU_ATTN_LONG"]
    assert k.kind == "user" and k.default == "1"
    assert knobs.check_environ({"KUNGFU_ATTN_LONG": "0"}) == []
    with open(os.path.join(ROOT, "docs", "KNOBS.md")) as f:
        assert "| `KUNGFU_ATTN_LONG` | `1` |" in f.read()
