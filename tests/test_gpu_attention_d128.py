"""GPU tests of the head dim 128 attention kernels (csrc/kernels/attention_d128.hip) on multi-head attention, their
instance with one head per group (the ``attention_d128_*`` bindings): bidirectional and causal, S = 64 .. 1024.

The reference is the float64 torch composition from the bf16 inputs (scale 1 / sqrt(128), the kernels' own dropout
mask); the yardstick is the same composition evaluated on bf16 tensors.  Errors are relative L2 per (sequence, head,
64-row block); the kernels' worst block must not exceed the yardstick's (margin 1.0: scores, softmax and the running
sums stay f32 in the kernels, only P and the outputs are rounded).
"""
import functools
import math

import pytest
import torch

from test_gpu_attention_long import BLOCK_BOUND, SEED, _hip

pytestmark = pytest.mark.gpu
needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

B, H, DH = 2, 2, 128
SCALE = 1.0 / math.sqrt(DH)


def _inputs(S):
    torch.manual_seed(41)
    qkv = (torch.randn(B, S, 3, H, DH, device="cuda") * 1.5).view(B, S, 3 * H * DH).bfloat16().contiguous()
    return qkv, torch.randn(B, S, H * DH, device="cuda").bfloat16()


def _run(qkv, gout, p, causal, seed=SEED):
    out, lse = _hip().attention_d128_forward(qkv, H, SCALE, seed, p, causal)
    return out, lse, _hip().attention_d128_backward(qkv, out, lse, gout, H, SCALE, seed, p, causal)


def composition(qkv, gout, p, causal, dtype):
    """(out [B, S, H*128], dqkv) of the torch composition in ``dtype`` with the kernels' dropout mask."""
    from kungfu_amd.ops import dropout_seed
    from kungfu_amd.ops.attention import dropout_keep

    S = qkv.shape[1]
    x = qkv.detach().to(dtype).requires_grad_(True)
    q, k, v = x.view(B, S, 3, H, DH).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) * SCALE
    if causal:
        s = s.masked_fill(torch.ones(S, S, dtype=torch.bool, device=qkv.device).triu(1), float("-inf"))
    keep = dropout_keep(dropout_seed.effective(SEED), B, H, S, p, device=qkv.device)
    out = ((torch.softmax(s, dim=-1) * keep.to(dtype) / (1 - p)) @ v).transpose(1, 2).reshape(B, S, H * DH)
    out.backward(gout.to(dtype))
    return out.detach(), x.grad


def _worst_block(got, ref, S):
    d = (got.double() - ref).view(B, S // 64, 64, H, DH).pow(2).sum((2, 4)).sqrt()
    return (d / ref.view(B, S // 64, 64, H, DH).pow(2).sum((2, 4)).sqrt()).max().item()


@functools.lru_cache(maxsize=None)
def _case(S, p, causal):
    from kungfu_amd.ops import dropout_seed

    dropout_seed.base("cuda")
    qkv, gout = _inputs(S)
    out, lse, dqkv = _run(qkv, gout, p, causal)
    return {"qkv": qkv, "gout": gout, "out": out, "lse": lse, "dqkv": dqkv}


@needs_gpu
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("S", [64, 128, 192, 1024])  # one block; first prefetch; ring slot reused; widest hash index
@pytest.mark.parametrize("causal", [False, True])
def test_matches_f64(causal, S, p):
    c = _case(S, p, causal)
    ref, rgrad = composition(c["qkv"], c["gout"], p, causal, torch.float64)
    yout, ygrad = composition(c["qkv"], c["gout"], p, causal, torch.bfloat16)
    g, y, r = (t.view(B, S, 3, H * DH) for t in (c["dqkv"], ygrad, rgrad))
    fails = []
    for name, got, yard, want in [("out", c["out"], yout, ref)] + [
            (n, g[:, :, t].contiguous(), y[:, :, t].contiguous(), r[:, :, t].contiguous())
            for t, n in enumerate(("dq", "dk", "dv"))]:
        assert torch.isfinite(got.float()).all(), name
        e, ey = _worst_block(got, want, S), _worst_block(yard, want, S)
        print("d128 causal=%s S=%d p=%g %-3s worst block %.3e, bf16 composition %.3e, BLOCK_BOUND %.3e (%s)" % (
            causal, S, p, name, e, ey, BLOCK_BOUND[name], "within" if e <= BLOCK_BOUND[name] else "beyond"))
        if not e <= ey:
            fails.append((name, e, ey))
    assert not fails, fails
    if causal:  # one visible key: the softmax is one-hot there
        assert not r[:, 0, 0].any() and not g[:, 0, 0].any()


@needs_gpu
@pytest.mark.parametrize("S,L", [(128, 64), (512, 192)])
def test_prefix_is_bitwise_the_shorter_call(S, L):
    """Causal, p = 0.1, no gradient into rows >= L: the first L rows are bitwise the call on qkv[:, :L]."""
    qkv, gout = _inputs(S)
    gout[:, L:] = 0
    out, lse, dqkv = _run(qkv, gout, 0.1, True)
    o2, l2, d2 = _run(qkv[:, :L].contiguous(), gout[:, :L].contiguous(), 0.1, True)
    assert torch.equal(out[:, :L], o2) and torch.equal(lse[:, :, :L], l2) and torch.equal(dqkv[:, :L], d2)


@needs_gpu
def test_future_keys_cannot_leak():
    """Causal, S = 256, p = 0: K rows >= 130 set to 1e4 and V rows >= 130 to NaN leave out[:, :130] finite and
    bitwise unchanged (queries 128 and 129 share their wave's diagonal triangle with the NaN rows)."""
    c = _case(256, 0.0, True)
    x = c["qkv"].clone().view(B, 256, 3, H * DH)
    x[:, 130:, 1], x[:, 130:, 2] = 1e4, float("nan")
    out = _hip().attention_d128_forward(x.view(B, 256, 3 * H * DH), H, SCALE, SEED, 0.0, True)[0]
    assert torch.isfinite(out[:, :130].float()).all()
    assert torch.equal(out[:, :130], c["out"][:, :130])


@needs_gpu
def test_reproducible_and_dropout_hash():
    c = _case(192, 0.1, False)
    again = _run(c["qkv"], c["gout"], 0.1, False)
    assert all(torch.equal(a, c[k]) for a, k in zip(again, ("out", "lse", "dqkv")))
    assert not torch.equal(_run(c["qkv"], c["gout"], 0.1, False, seed=SEED + 1)[0], c["out"])


@needs_gpu
def test_public_route(monkeypatch):
    """self_attention routes head dim 128 to the new autograd function (not with lengths), and a 2-layer GPTLM with
    heads of 128 under bf16 autocast is as close to the model without the fused attention (the module switch
    ``ops.attention._D128_ENABLED``) as that model is to an f32 run of the same weights."""
    from kungfu_amd.models.gpt import GPTLM
    from kungfu_amd.ops import attention as attn

    qkv = torch.randn(1, 128, 3 * 2 * DH, device="cuda").bfloat16().requires_grad_(True)
    for causal in (False, True):
        assert type(attn.self_attention(qkv, 2, causal=causal).grad_fn).__name__ == "_AttnD128FnBackward"
    lens = torch.full((1,), 100, dtype=torch.int32, device="cuda")
    assert type(attn.self_attention(qkv, 2, 0.0, lens).grad_fn).__name__ != "_AttnD128FnBackward"

    torch.manual_seed(5)
    model = GPTLM(vocab=512, d=256, layers=2, heads=2, ffn=512, max_pos=128).cuda().eval()
    ids = torch.randint(0, 512, (2, 128), device="cuda")
    with torch.no_grad():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            fused = model(ids).float()
            monkeypatch.setattr(attn, "_D128_ENABLED", False)
            sdpa = model(ids).float()
        f32 = model(ids).float()
    d_fused, d_sdpa = (fused - sdpa).norm() / f32.norm(), (sdpa - f32).norm() / f32.norm()
    print("GPT d128 x 2: fused vs sdpa %.3e, sdpa vs f32 %.3e" % (d_fused, d_sdpa))
    assert d_fused <= d_sdpa


@needs_gpu
@pytest.mark.parametrize("case", ["head dim 64", "S = 96", "S = 1088", "f32", "out shape"])
def test_binding_refusals(case):
    S = {"S = 96": 96, "S = 1088": 1088}.get(case, 128)
    qkv = torch.zeros(1, S, 3 * 2 * (64 if case == "head dim 64" else DH), device="cuda",
                      dtype=torch.float32 if case == "f32" else torch.bfloat16)
    with pytest.raises(RuntimeError, match="attention_d128_"):
        if case == "out shape":
            out, lse = _hip().attention_d128_forward(qkv, 2, SCALE, 1, 0.0)
            _hip().attention_d128_backward(qkv, out[:, :, :DH].contiguous(), lse, out, 2, SCALE, 1, 0.0)
        else:
            _hip().attention_d128_forward(qkv, 2, SCALE, 1, 0.0)
