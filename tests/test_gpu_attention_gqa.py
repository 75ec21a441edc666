"""GPU tests of the head dim 128 attention kernels (csrc/kernels/attention_d128.hip) on grouped-query heads (the
``attention_gqa_*`` bindings): qkv [B, S, (H + 2*Hkv)*128], bidirectional and causal, S = 64 .. 1024.

The reference is the float64 torch composition from the bf16 inputs (K/V expanded with repeat_interleave, so autograd
sums each group's dk / dv; scale 1 / sqrt(128); the kernels' own dropout mask, keyed on the query head); the yardstick
is the same composition evaluated on bf16 tensors.  Errors are relative L2 per (sequence, head, 64-row block), dk and
dv per K/V head; the kernels' worst block must not exceed the yardstick's (margin 1.0), as in
test_gpu_attention_d128.py.
"""
import functools
import math

import pytest
import torch

from test_gpu_attention_long import BLOCK_BOUND, SEED, _hip

pytestmark = pytest.mark.gpu
needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

B, DH = 2, 128
SCALE = 1.0 / math.sqrt(DH)


def _inputs(S, H, Hkv):
    torch.manual_seed(41)
    qkv = (torch.randn(B, S, (H + 2 * Hkv) * DH, device="cuda") * 1.5).bfloat16().contiguous()
    return qkv, torch.randn(B, S, H * DH, device="cuda").bfloat16()


def _run(qkv, gout, H, Hkv, p, causal, seed=SEED):
    out, lse = _hip().attention_gqa_forward(qkv, H, Hkv, SCALE, seed, p, causal)
    return out, lse, _hip().attention_gqa_backward(qkv, out, lse, gout, H, Hkv, SCALE, seed, p, causal)


def _parts(x, H, Hkv):
    """The (q, k, v) column ranges of a [B, S, (H + 2*Hkv)*128] tensor."""
    return x.split((H * DH, Hkv * DH, Hkv * DH), dim=2)


def _expanded(qkv, H, Hkv):
    """(q, k, v) as [B, S, H, 128] each: query head h next to its K/V head h // G."""
    S = qkv.shape[1]
    q, k, v = _parts(qkv, H, Hkv)
    k, v = (t.view(B, S, Hkv, DH).repeat_interleave(H // Hkv, dim=2) for t in (k, v))
    return q.view(B, S, H, DH), k, v


def composition(qkv, gout, H, Hkv, p, causal, dtype):
    """(out [B, S, H*128], dqkv) of the torch composition in ``dtype`` with the kernels' dropout mask."""
    from kungfu_amd.ops import dropout_seed
    from kungfu_amd.ops.attention import dropout_keep

    S = qkv.shape[1]
    x = qkv.detach().to(dtype).requires_grad_(True)
    q, k, v = (t.transpose(1, 2) for t in _expanded(x, H, Hkv))
    s = q @ k.transpose(-1, -2) * SCALE
    if causal:
        s = s.masked_fill(torch.ones(S, S, dtype=torch.bool, device=qkv.device).triu(1), float("-inf"))
    keep = dropout_keep(dropout_seed.effective(SEED), B, H, S, p, device=qkv.device)
    out = ((torch.softmax(s, dim=-1) * keep.to(dtype) / (1 - p)) @ v).transpose(1, 2).reshape(B, S, H * DH)
    out.backward(gout.to(dtype))
    return out.detach(), x.grad


def _worst_block(got, ref):
    S, heads = ref.shape[1], ref.shape[2] // DH
    d = (got.double() - ref).view(B, S // 64, 64, heads, DH).pow(2).sum((2, 4)).sqrt()
    return (d / ref.view(B, S // 64, 64, heads, DH).pow(2).sum((2, 4)).sqrt()).max().item()


@functools.lru_cache(maxsize=None)
def _case(S, H, Hkv, p, causal):
    from kungfu_amd.ops import dropout_seed

    dropout_seed.base("cuda")
    qkv, gout = _inputs(S, H, Hkv)
    out, lse, dqkv = _run(qkv, gout, H, Hkv, p, causal)
    return {"qkv": qkv, "gout": gout, "out": out, "lse": lse, "dqkv": dqkv}


# S = 64: one block, the head switch is the stream's first prefetch; 128: a prefetch inside a head and across one;
# 192: a ring slot reused across a head boundary, an odd number of steps per head; 1024: the widest hash index
CASES = [(c, hh, p, S) for c in (False, True) for hh in ((4, 2), (4, 1)) for p in (0.0, 0.1) for S in (64, 128, 192)]


@needs_gpu
@pytest.mark.parametrize("causal,heads,p,S", CASES + [(True, (4, 2), 0.1, 1024)])
def test_matches_f64(causal, heads, p, S):
    H, Hkv = heads
    c = _case(S, H, Hkv, p, causal)
    ref, rgrad = composition(c["qkv"], c["gout"], H, Hkv, p, causal, torch.float64)
    yout, ygrad = composition(c["qkv"], c["gout"], H, Hkv, p, causal, torch.bfloat16)
    g, y, r = (_parts(t, H, Hkv) for t in (c["dqkv"], ygrad, rgrad))
    fails = []
    for name, got, yard, want in [("out", c["out"], yout, ref)] + [
            (n, g[t].contiguous(), y[t].contiguous(), r[t].contiguous()) for t, n in enumerate(("dq", "dk", "dv"))]:
        assert torch.isfinite(got.float()).all(), name
        e, ey = _worst_block(got, want), _worst_block(yard, want)
        print("gqa causal=%s H=%d Hkv=%d S=%d p=%g %-3s worst block %.3e, bf16 composition %.3e, BLOCK_BOUND %.3e (%s)"
              % (causal, H, Hkv, S, p, name, e, ey, BLOCK_BOUND[name], "within" if e <= BLOCK_BOUND[name] else "beyond"))
        if not e <= ey:
            fails.append((name, e, ey))
    assert not fails, fails
    if causal:  # one visible key: the softmax is one-hot there
        assert not r[0][:, 0].any() and not g[0][:, 0].any()


def _bf16_ulp(x):
    """One unit in the last place of bf16 (8 significand bits) at the magnitude of the f32 tensor x."""
    return torch.ldexp(torch.ones_like(x), torch.frexp(x)[1] - 8)


@needs_gpu
@pytest.mark.parametrize("causal", [False, True])
def test_equals_d128_on_expanded_kv(causal):
    """(4, 2), S = 192, p = 0.1 against attention_d128_* on K/V expanded to 4 heads: out, lse and dq bitwise (the same
    arithmetic per query head, the same hash); dk / dv within one bf16 ulp of the f32 sum of the expanded call's
    per-head gradients, each of which was rounded to bf16 (the ulp taken at the largest of the two addends and the
    result: the addends may cancel)."""
    H, Hkv, S = 4, 2, 192
    c = _case(S, H, Hkv, 0.1, causal)
    x = torch.stack(_expanded(c["qkv"], H, Hkv), dim=2).reshape(B, S, 3 * H * DH).contiguous()
    out, lse = _hip().attention_d128_forward(x, H, SCALE, SEED, 0.1, causal)
    dx = _hip().attention_d128_backward(x, out, lse, c["gout"], H, SCALE, SEED, 0.1, causal).view(B, S, 3, H * DH)
    dq, dk, dv = _parts(c["dqkv"], H, Hkv)
    assert torch.equal(out, c["out"]) and torch.equal(lse, c["lse"]) and torch.equal(dx[:, :, 0], dq)
    for name, t, got in (("dk", 1, dk), ("dv", 2, dv)):
        addends = dx[:, :, t].float().view(B, S, Hkv, H // Hkv, DH)
        ulp = _bf16_ulp(torch.maximum(addends.abs().amax(3), got.float().view(B, S, Hkv, DH).abs()))
        worst = ((got.float().view(B, S, Hkv, DH) - addends.sum(3)).abs() / ulp).max().item()
        print("gqa vs expanded d128 causal=%s %s: worst element %.3f bf16 ulp" % (causal, name, worst))
        assert worst <= 1.0, (name, worst)


@needs_gpu
def test_g1_is_bitwise_d128():
    """kv_heads == heads: the d128 layout, and the attention_d128_* bindings' results bit for bit (S = 192, causal,
    p = 0.1).  Both run the same kernels at G = 1, so this pins the bindings' plumbing (Hkv = H, no tables)."""
    qkv, gout = _inputs(192, 2, 2)
    out, lse = _hip().attention_d128_forward(qkv, 2, SCALE, SEED, 0.1, True)
    dqkv = _hip().attention_d128_backward(qkv, out, lse, gout, 2, SCALE, SEED, 0.1, True)
    assert all(torch.equal(a, b) for a, b in zip(_run(qkv, gout, 2, 2, 0.1, True), (out, lse, dqkv)))


@needs_gpu
@pytest.mark.parametrize("S,L", [(128, 64), (512, 192)])
def test_prefix_is_bitwise_the_shorter_call(S, L):
    """Causal, (4, 1), p = 0.1, no gradient into rows >= L: the first L rows are bitwise the call on qkv[:, :L]."""
    qkv, gout = _inputs(S, 4, 1)
    gout[:, L:] = 0
    out, lse, dqkv = _run(qkv, gout, 4, 1, 0.1, True)
    o2, l2, d2 = _run(qkv[:, :L].contiguous(), gout[:, :L].contiguous(), 4, 1, 0.1, True)
    assert torch.equal(out[:, :L], o2) and torch.equal(lse[:, :, :L], l2) and torch.equal(dqkv[:, :L], d2)


@needs_gpu
def test_future_keys_cannot_leak():
    """Causal, (4, 2), S = 256, p = 0: K rows >= 130 set to 1e4 and V rows >= 130 to NaN leave out[:, :130] finite and
    bitwise unchanged (queries 128 and 129 share their wave's diagonal triangle with the NaN rows)."""
    H, Hkv = 4, 2
    c = _case(256, H, Hkv, 0.0, True)
    x = c["qkv"].clone()
    x[:, 130:, H * DH:(H + Hkv) * DH], x[:, 130:, (H + Hkv) * DH:] = 1e4, float("nan")
    out = _hip().attention_gqa_forward(x, H, Hkv, SCALE, SEED, 0.0, True)[0]
    assert torch.isfinite(out[:, :130].float()).all()
    assert torch.equal(out[:, :130], c["out"][:, :130])


@needs_gpu
def test_reproducible():
    c = _case(192, 4, 2, 0.1, False)
    again = _run(c["qkv"], c["gout"], 4, 2, 0.1, False)
    assert all(torch.equal(a, c[k]) for a, k in zip(again, ("out", "lse", "dqkv")))
    assert not torch.equal(_run(c["qkv"], c["gout"], 4, 2, 0.1, False, seed=SEED + 1)[0], c["out"])


@needs_gpu
def test_public_route(monkeypatch):
    """self_attention routes kv_heads at head dim 128 to the new autograd function and leaves the call without it
    alone, and a 2-layer grouped-query GPTLM under bf16 autocast is as close to the model without the fused attention
    (the module switch ``ops.attention._GQA_ENABLED``) as that model is to an f32 run of the same weights."""
    from kungfu_amd.models.gpt import GPTLM
    from kungfu_amd.ops import attention as attn

    qkv = torch.randn(1, 128, 8 * DH, device="cuda").bfloat16().requires_grad_(True)
    for causal in (False, True):
        assert type(attn.self_attention(qkv, 4, causal=causal, kv_heads=2).grad_fn).__name__ == "_AttnGQAFnBackward"
    plain = torch.randn(1, 128, 12 * DH, device="cuda").bfloat16().requires_grad_(True)
    assert type(attn.self_attention(plain, 4, kv_heads=None).grad_fn).__name__ == "_AttnD128FnBackward"
    with pytest.raises(ValueError):
        attn.self_attention(qkv, 4, 0.0, torch.full((1,), 100, dtype=torch.int32, device="cuda"), kv_heads=2)

    torch.manual_seed(5)
    model = GPTLM(vocab=512, d=512, layers=2, heads=4, kv_heads=2, ffn=512, max_pos=128).cuda().eval()
    ids = torch.randint(0, 512, (2, 128), device="cuda")
    with torch.no_grad():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            fused = model(ids).float()
            monkeypatch.setattr(attn, "_GQA_ENABLED", False)
            sdpa = model(ids).float()
        f32 = model(ids).float()
    d_fused, d_sdpa = (fused - sdpa).norm() / f32.norm(), (sdpa - f32).norm() / f32.norm()
    print("GPT gqa x 2: fused vs sdpa %.3e, sdpa vs f32 %.3e" % (d_fused, d_sdpa))
    assert d_fused <= d_sdpa


@needs_gpu
@pytest.mark.parametrize("case", ["H % Hkv", "head dim 64", "S = 96", "S = 1088", "f32", "out shape"])
def test_binding_refusals(case):
    S = {"S = 96": 96, "S = 1088": 1088}.get(case, 128)
    Hkv = 3 if case == "H % Hkv" else 2
    qkv = torch.zeros(1, S, (4 + 2 * Hkv) * (64 if case == "head dim 64" else DH), device="cuda",
                      dtype=torch.float32 if case == "f32" else torch.bfloat16)
    with pytest.raises(RuntimeError, match="attention_gqa_"):
        if case == "out shape":
            out, lse = _hip().attention_gqa_forward(qkv, 4, Hkv, SCALE, 1, 0.0)
            _hip().attention_gqa_backward(qkv, out[:, :, :DH].contiguous(), lse, out, 4, Hkv, SCALE, 1, 0.0)
        else:
            _hip().attention_gqa_forward(qkv, 4, Hkv, SCALE, 1, 0.0)
