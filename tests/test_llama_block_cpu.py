"""CPU tests of the fallbacks of ops/rmsnorm.py and ops/swiglu.py and of the ``llama`` model's structure."""
import pytest
import torch

from kungfu_amd.models import get_model
from kungfu_amd.models.bert import BertLayer
from kungfu_amd.models.gpt import GPTLM, lm_loss, synthetic_lm_batch
from kungfu_amd.ops.rmsnorm import AddRMSNorm, add_rms_norm
from kungfu_amd.ops.swiglu import swiglu
from kungfu_amd.utils.numerics import rel_err

EPS = 1e-6


def _rms_f64(x, r, w):
    s = x.double() if r is None else x.double() + r.double()
    return s * torch.rsqrt(s.pow(2).mean(-1, keepdim=True) + EPS) * w.double(), s


@pytest.mark.parametrize("with_r", [True, False])
def test_rmsnorm_fallback_matches_definition(with_r):
    torch.manual_seed(0)
    x, r, w = torch.randn(3, 5, 48), torch.randn(3, 5, 48) if with_r else None, torch.randn(48)
    (y, s), (ry, rs) = add_rms_norm(x, r, w, EPS), _rms_f64(x, r, w)
    assert y.dtype == s.dtype == torch.float32 and (with_r or s is x)
    assert rel_err(ry, y) <= 1e-5 and rel_err(rs, s) <= 1e-5
    m = AddRMSNorm(48, EPS)
    assert [n for n, _ in m.named_parameters()] == ["weight"] and torch.equal(m.weight, torch.ones(48))
    assert torch.equal(m(x, r)[0], add_rms_norm(x, r, torch.ones(48), EPS)[0])


def test_swiglu_fallback_matches_definition():
    torch.manual_seed(0)
    gu = torch.randn(2, 7, 32) * 3
    g, u = gu[..., :16].double(), gu[..., 16:].double()
    h = swiglu(gu)
    assert h.shape == (2, 7, 16) and h.dtype == torch.float32 and rel_err(g * torch.sigmoid(g) * u, h) <= 1e-5
    with pytest.raises(ValueError):
        swiglu(torch.randn(2, 7))


def test_gradcheck():
    torch.manual_seed(0)
    x, r, w = (torch.randn(*s, dtype=torch.float64, requires_grad=True) for s in ((3, 8), (3, 8), (8,)))
    assert torch.autograd.gradcheck(lambda a, b, c: add_rms_norm(a, b, c, EPS), (x, r, w))
    assert torch.autograd.gradcheck(lambda a, c: add_rms_norm(a, None, c, EPS)[0], (x, w))
    assert torch.autograd.gradcheck(swiglu, (torch.randn(3, 16, dtype=torch.float64, requires_grad=True),))


def test_llama_model_structure():
    torch.manual_seed(0)
    m = get_model("llama", vocab=50, d=64, layers=2, heads=2, kv_heads=1, ffn=48)
    layer = ["norm1.weight", "qkv.weight", "out.weight", "norm2.weight", "gate_up.weight", "down.weight"]
    assert list(m.state_dict()) == ["tok.weight"] + ["layers.%d.%s" % (i, n) for i in (0, 1) for n in layer] + [
        "norm.weight"]
    assert m.layers[0].qkv.weight.shape == (128, 64) and m.layers[0].gate_up.weight.shape == (96, 64)
    assert not any("bias" in n or "pos" in n for n in m.state_dict())
    loss = lm_loss(m, synthetic_lm_batch(2, 16, 50))
    loss.backward()
    assert torch.isfinite(loss) and all(p.grad is not None and p.grad.abs().sum() > 0 for p in m.parameters())


def test_bert_and_gpt_parameters_unchanged():
    names = ["qkv", "out", "ln1", "fc1", "fc2", "ln2"]
    assert [n for n, _ in BertLayer().named_parameters()] == ["%s.%s" % (n, p) for n in names for p in ("weight", "bias")]
    assert {n: tuple(p.shape) for n, p in BertLayer().named_parameters() if n.endswith("weight")} == {
        "qkv.weight": (2304, 768), "out.weight": (768, 768), "ln1.weight": (768,), "fc1.weight": (3072, 768),
        "fc2.weight": (768, 3072), "ln2.weight": (768,)}
    g = GPTLM(vocab=64, layers=1)
    assert list(g.state_dict())[:2] == ["tok.weight", "pos.weight"] and g.pos.weight.shape == (512, 768)
    assert len(g.state_dict()) == 2 + 12
