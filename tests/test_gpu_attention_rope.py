"""GPU tests of rotary position embeddings at head dim 128: csrc/kernels/attention_rope.hip and the ROPE epilogues of
attention_d128.hip.  B = 2, inputs 1.5 x randn in bf16, base 10000, the tables of ops.attention.rope_tables; block
errors and their yardstick (the same composition in bf16) as in test_gpu_attention_gqa.py."""
import functools

import pytest
import torch

from kungfu_amd.models import get_model
from kungfu_amd.models.gpt import lm_loss
from kungfu_amd.ops import attention as attn, dropout_seed
from test_gpu_attention_gqa import B, DH, SCALE, _bf16_ulp, _inputs, _parts, _worst_block, composition
from test_gpu_attention_long import SEED, _hip

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]


def _tables(S):
    return attn.rope_tables(S, 10000.0, "cuda")


def _halves(x, H, Hkv):
    """(lower halves of the Q and K heads, their upper halves, the V heads) of a [B, S, (H + 2*Hkv)*128] tensor."""
    h = x.view(B, x.shape[1], H + 2 * Hkv, DH)
    return h[:, :, :H + Hkv, :64], h[:, :, :H + Hkv, 64:], h[:, :, H + Hkv:]


def _rotate(x, H, Hkv, transposed=False):
    """The definition in x's dtype from the f32 tables; ``transposed``: the gradient's rotation (sin -> -sin)."""
    lo, hi, v = _halves(x, H, Hkv)
    c, s = (t.to(x.dtype)[None, :, None] for t in _tables(x.shape[1]))
    s = -s if transposed else s
    return torch.cat((torch.cat((lo * c - hi * s, hi * c + lo * s), 3), v), 2).view(x.shape)


@functools.lru_cache(maxsize=None)
def _case(S, H, Hkv, p, causal):
    """The kernels' results and the float64 / bf16 compositions (rotation included) of one shape."""
    dropout_seed.base("cuda")
    qkv, gout = _inputs(S, H, Hkv)
    cos, sin = _tables(S)
    rot = _hip().rope_forward(qkv, H, Hkv, cos, sin)
    out, lse = _hip().attention_gqa_forward(rot, H, Hkv, SCALE, SEED, p, causal)
    back = (rot, out, lse, gout, H, Hkv, SCALE, SEED, p, causal)
    c = {"qkv": qkv, "gout": gout, "out": out, "back": back, "plain": _hip().attention_gqa_backward(*back),
         "dqkv": _hip().attention_gqa_backward(*back, cos=cos, sin=sin)}
    for name, dtype in (("ref", torch.float64), ("yard", torch.bfloat16)):
        o, g = composition(_rotate(qkv.to(dtype), H, Hkv), gout, H, Hkv, p, causal, dtype)
        c[name] = (o, _rotate(g, H, Hkv, transposed=True))
    return c


def _block_errors(c, got_out, got_grad, H, Hkv):
    """[(name, worst block of the result, worst block of the bf16 composition)] against the float64 composition."""
    (ro, rg), (yo, yg) = c["ref"], c["yard"]
    g, y, r = ([t.contiguous() for t in _parts(x, H, Hkv)] for x in (got_grad, yg, rg))
    return [("out", _worst_block(got_out, ro), _worst_block(yo, ro))] + [
        (n, _worst_block(g[t], r[t]), _worst_block(y[t], r[t])) for t, n in enumerate(("dq", "dk", "dv"))]


@pytest.mark.parametrize("S", [64, 1024])
@pytest.mark.parametrize("heads", [(4, 2), (2, 2), (4, 1)])
def test_rope_forward_matches_f64(heads, S):
    """One rounding plus the f32 arithmetic (it matters where the products cancel); V and row 0 bitwise the input."""
    H, Hkv = heads
    (qkv, _), (cos, sin) = _inputs(S, H, Hkv), _tables(S)
    (glo, ghi, gv), (lo, hi, v) = _halves(_hip().rope_forward(qkv, H, Hkv, cos, sin), H, Hkv), _halves(qkv, H, Hkv)
    assert torch.equal(gv, v) and torch.equal(glo[:, 0], lo[:, 0]) and torch.equal(ghi[:, 0], hi[:, 0])
    elo, ehi, _ = _halves(_rotate(qkv.double(), H, Hkv), H, Hkv)
    c, s, lo, hi = (t.double().abs() for t in (cos[None, :, None], sin[None, :, None], lo, hi))
    for g, e, mag in ((glo.double(), elo, lo * c + hi * s), (ghi.double(), ehi, hi * c + lo * s)):
        bound = 0.5 * _bf16_ulp(torch.maximum(g.abs(), e.abs())) + 2.0 ** -22 * mag
        assert ((g - e).abs() <= bound).all(), ((g - e).abs() / bound).max().item()


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("heads", [(4, 2), (2, 2)])
def test_backward_epilogue_elementwise(heads, causal):
    """Against the call without tables rotated back in f64: dv, row 0 bitwise; dq, dk within 2 u, u one bf16 ulp at
    max(|dx'[i]|, |dx'[i + 64]|) (unfused operands: 0.5 ulp each x (|c| + |s| <= sqrt 2); fused: one rounding <= 1 u)."""
    H, Hkv = heads
    c = _case(192, H, Hkv, 0.1, causal)
    (glo, ghi, gv), (plo, phi, pv) = _halves(c["dqkv"], H, Hkv), _halves(c["plain"], H, Hkv)
    assert torch.equal(gv, pv) and torch.equal(glo[:, 0], plo[:, 0]) and torch.equal(ghi[:, 0], phi[:, 0])
    wlo, whi, _ = _halves(_rotate(c["plain"].double(), H, Hkv, transposed=True), H, Hkv)
    u = _bf16_ulp(torch.maximum(plo.double().abs(), phi.double().abs()))
    worst = [((g.double() - w).abs() / u).max().item() for g, w in ((glo, wlo), (ghi, whi))]
    print("rope epilogue H=%d Hkv=%d causal=%s: worst lower / upper half %.3f / %.3f u" % (H, Hkv, causal, *worst))
    assert max(worst) <= 2.0, worst


@pytest.mark.parametrize("causal,heads,S", [(c, hh, S) for c in (False, True) for hh in ((4, 2), (2, 2))
                                            for S in (64, 192)] + [(True, (4, 2), 1024)])
def test_matches_f64_composition(causal, heads, S):
    c = _case(S, *heads, 0.1, causal)
    errs = _block_errors(c, c["out"], c["dqkv"], *heads)
    print("rope causal=%s heads=%s S=%d: (name, worst block, bf16 composition) %s" % (causal, heads, S, errs))
    assert all(e <= y for _, e, y in errs), errs  # (a NaN fails the comparison)


def test_public_route(monkeypatch):
    H, Hkv, S = 4, 2, 64
    c, res = _case(S, H, Hkv, 0.0, True), []
    for enabled in (True, False):
        monkeypatch.setattr(attn, "_ROPE_ENABLED", enabled)
        x = c["qkv"].clone().requires_grad_(True)
        y = attn.self_attention(x, H, 0.0, causal=True, kv_heads=Hkv, rope=10000.0)
        assert (type(y.grad_fn).__name__ == "_AttnRopeFnBackward") == enabled
        res.append((y.detach(), torch.autograd.grad(y, x, c["gout"])[0]))
    assert torch.equal(res[0][0], c["out"]) and torch.equal(res[0][1], c["dqkv"])
    new, old = ((o, *_parts(g, H, Hkv)) for o, g in res)  # the routes differ by less than the bf16 composition's error
    for (name, _, y), a, b in zip(_block_errors(c, *res[0], H, Hkv), new, old):
        assert _worst_block(a.contiguous(), b.contiguous().double()) <= y, name
    monkeypatch.setattr(attn, "_ROPE_ENABLED", True)
    model = get_model("gpt_rope", vocab=512, d=256, layers=2, heads=2, kv_heads=1, ffn=512).cuda()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        lm_loss(model, torch.randint(0, 512, (2, S), device="cuda")).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())


@pytest.mark.parametrize("case", ["a row too few", "f64", "cpu", "cos only"])
def test_binding_refusals(case):
    c = _case(64, 4, 2, 0.0, True)
    spoil = {"a row too few": lambda t: t[:-1], "f64": lambda t: t.double(), "cpu": lambda t: t.cpu()}
    cos, sin = (spoil.get(case, lambda t: t)(t) for t in _tables(64))
    with pytest.raises(RuntimeError, match="attention_gqa_backward: .*(cos|sin)"):
        _hip().attention_gqa_backward(*c["back"], cos=cos, **({} if case == "cos only" else {"sin": sin}))
    if case != "cos only":
        with pytest.raises(RuntimeError, match="rope_forward: cos"):
            _hip().rope_forward(c["qkv"], 4, 2, cos, sin)
