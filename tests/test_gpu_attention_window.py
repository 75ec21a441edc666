"""GPU tests of sliding-window causal attention at head dim 128 (the BAND kernels of csrc/kernels/attention_d128.hip,
``window`` of the ``attention_gqa_*`` bindings), S up to 8192.  Reference: the float64 torch composition with the band
mask q - W < k <= q and the kernels' dropout mask; yardstick: the same composition on bf16 tensors, per (sequence,
head, 64-row block), margin 1.0: the rule and the reason of test_gpu_attention_gqa.py."""
import pytest
import torch

from kungfu_amd.ops import attention as attn, dropout_seed
from test_gpu_attention_gqa import DH, SCALE, _inputs, _parts
from test_gpu_attention_long import SEED, _hip
from test_gpu_attention_rope import _rotate, _tables

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]


def _run(qkv, gout, H, Hkv, p, window, rope=False, causal=True):
    """(out, lse, dqkv) of the bindings; ``rope``: behind rope_forward, the rotation undone in the epilogues."""
    kw = dict(zip(("cos", "sin"), _tables(qkv.shape[1]))) if rope else {}
    x = _hip().rope_forward(qkv, H, Hkv, *kw.values()) if rope else qkv
    out, lse = _hip().attention_gqa_forward(x, H, Hkv, SCALE, SEED, p, causal, window)
    return out, lse, _hip().attention_gqa_backward(x, out, lse, gout, H, Hkv, SCALE, SEED, p, causal, window=window, **kw)


def _composition(qkv, gout, H, Hkv, p, W, dtype, rope=False, start=0):
    """(out, dqkv) in ``dtype``; ``start``: qkv holds rows start .. of a longer sequence (the hash's global indices)."""
    (Bx, S), x = qkv.shape[:2], qkv.detach().to(dtype).requires_grad_(True)
    q, k, v = _parts(_rotate(x, H, Hkv) if rope else x, H, Hkv)
    q = q.view(Bx, S, H, DH).transpose(1, 2)
    k, v = (t.view(Bx, S, Hkv, DH).transpose(1, 2).repeat_interleave(H // Hkv, dim=1) for t in (k, v))
    d = torch.arange(S, device=qkv.device)[:, None] - torch.arange(S, device=qkv.device)[None, :]  # query - key
    s = (q @ k.transpose(-1, -2) * SCALE).masked_fill((d < 0) | (d >= W), float("-inf"))
    keep = attn.dropout_keep(dropout_seed.effective(SEED), Bx, H, S, p, device=qkv.device, start=start)
    out = ((torch.softmax(s, dim=-1) * keep.to(dtype) / (1 - p)) @ v).transpose(1, 2).reshape(Bx, S, H * DH)
    out.backward(gout.to(dtype))
    return out.detach(), x.grad


def _worst_block(got, ref):
    shape = (ref.shape[0], ref.shape[1] // 64, 64, ref.shape[2] // DH, DH)
    d = (got.double() - ref).reshape(shape).pow(2).sum((2, 4)).sqrt()
    return (d / ref.reshape(shape).pow(2).sum((2, 4)).sqrt()).max().item()


def _check(tag, got, yard, ref, H, Hkv):
    """out, dq, dk, dv of (out, dqkv) triples: finite, and no block worse than the bf16 composition's worst."""
    for t, name in enumerate(("out", "dq", "dk", "dv")):
        g, y, r = (x[0] if t == 0 else _parts(x[1], H, Hkv)[t - 1] for x in (got, yard, ref))
        assert torch.isfinite(g.float()).all(), name
        e, ey = _worst_block(g, r), _worst_block(y, r)
        print("window %s %-3s worst block %.3e, bf16 composition %.3e" % (tag, name, e, ey))
        assert e <= ey, (name, e, ey)


# (128, 64): block 0 without an edge block, block 1 with one, nothing unmasked; (192, 64): a key block that drops out
# of view, `first` odd and even; (256, 128): one unmasked block between edge and diagonal, dK/dV streams that end at the
# edge and at n - 1; (1152, 128): rope, past the S of the calls without a window
@pytest.mark.parametrize("S,W,rope", [(128, 64, False), (192, 64, False), (256, 128, False), (1152, 128, True)])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("heads", [(4, 2), (4, 1)])
def test_matches_f64(heads, p, S, W, rope):
    H, Hkv = heads
    dropout_seed.base("cuda")
    qkv, gout = _inputs(S, H, Hkv)
    out, _, dqkv = _run(qkv, gout, H, Hkv, p, W, rope)
    ref, yard = (_composition(qkv, gout, H, Hkv, p, W, dt, rope) for dt in (torch.float64, torch.bfloat16))
    _check("H=%d Hkv=%d S=%d W=%d p=%g rope=%d" % (H, Hkv, S, W, p, rope), (out, dqkv), yard, ref, H, Hkv)


@pytest.mark.parametrize("window", [192, 1024])
def test_window_at_least_S_is_bitwise_causal(window):
    """No edge block anywhere (w >= n): the band instantiations' out, lse and dqkv are the causal call's bit for bit."""
    qkv, gout = _inputs(192, 4, 2)
    assert all(torch.equal(a, b) for a, b in zip(_run(qkv, gout, 4, 2, 0.1, window), _run(qkv, gout, 4, 2, 0.1, 0)))


def test_longest_S():
    """The last 64 rows at S = 8192, W = 64 against the composition on rows S - 128 .. S - 1 (those queries see no
    earlier key and no other query sees those keys), global hash indices."""
    H, Hkv, S = 2, 1, 8192
    dropout_seed.base("cuda")
    torch.manual_seed(43)
    qkv = (torch.randn(1, S, (H + 2 * Hkv) * DH, device="cuda") * 1.5).bfloat16()
    gout = torch.randn(1, S, H * DH, device="cuda").bfloat16()
    out, _, dqkv = _run(qkv, gout, H, Hkv, 0.1, 64)
    ref, yard = (_composition(qkv[:, -128:], gout[:, -128:], H, Hkv, 0.1, 64, dt, start=S - 128)
                 for dt in (torch.float64, torch.bfloat16))
    _check("S=8192 W=64 last block", (out[:, -64:], dqkv[:, -64:]), [t[:, -64:] for t in yard],
           [t[:, -64:] for t in ref], H, Hkv)


def test_routes(monkeypatch):
    """The new autograd node with and without kv_heads and rope, the fallback with the switch off, and a 2-layer
    LlamaLM(window=128) under bf16 autocast as close to itself on the fallback as that one is to its f32 run."""
    from kungfu_amd.models.llama import LlamaLM
    for kv, rope in ((None, None), (2, None), (None, 10000.0), (2, 10000.0)):
        x = torch.randn(1, 256, (4 + 2 * (kv or 4)) * DH, device="cuda").bfloat16().requires_grad_(True)
        for enabled in (True, False):
            monkeypatch.setattr(attn, "_WINDOW_ENABLED", enabled)
            y = attn.self_attention(x, 4, causal=True, kv_heads=kv, rope=rope, window=128)
            assert (type(y.grad_fn).__name__ == "_AttnWindowFnBackward") == enabled, (kv, rope, enabled)
    torch.manual_seed(5)
    model = LlamaLM(vocab=512, d=512, layers=2, heads=4, kv_heads=2, ffn=512, window=128).cuda().eval()
    ids = torch.randint(0, 512, (2, 256), device="cuda")
    with torch.no_grad():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            sdpa = model(ids).float()
            monkeypatch.setattr(attn, "_WINDOW_ENABLED", True)
            fused = model(ids).float()
        f32 = model(ids).float()
    d_fused, d_sdpa = (fused - sdpa).norm() / f32.norm(), (sdpa - f32).norm() / f32.norm()
    print("Llama window x 2: fused vs sdpa %.3e, sdpa vs f32 %.3e" % (d_fused, d_sdpa))
    assert d_fused <= d_sdpa


@pytest.mark.parametrize("S,window,causal,match", [(128, 96, True, "window"), (128, 64, False, "window"),
                                                   (8256, 64, True, "window"), (1088, 0, True, "qkv must be")])
def test_binding_refusals(S, window, causal, match):
    qkv = torch.zeros(1, S, 8 * DH, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="attention_gqa_forward: .*" + match):
        _hip().attention_gqa_forward(qkv, 4, 2, SCALE, 1, 0.0, causal, window)
