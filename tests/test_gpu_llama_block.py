"""GPU tests of csrc/kernels/rmsnorm.hip and swiglu.hip, element by element against float64, of the routes of
ops/rmsnorm.py and ops/swiglu.py, and of the ``llama`` model against the same model in float64.  U = 2^-24, one f32
rounding; every ``assert_rounds_from`` also asserts, on the reference alone, that at most 1 % of the elements sit on a
rounding boundary (a condition on the data and seeds chosen here, not on the kernel)."""
import functools
import itertools

import pytest
import torch

from kungfu_amd._lib import hip
from kungfu_amd.models import get_model
from kungfu_amd.models.gpt import lm_loss, synthetic_lm_batch
from kungfu_amd.ops import rmsnorm as rn, swiglu as sw
from kungfu_amd.utils.numerics import assert_rounds_from, integer_data, rel_err, ulp_of

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

U, EPS = 2.0 ** -24, 1e-6
CROSS = 2304  # the first row length on the workgroup-per-row scheme
PAST_CAP = 32768 + 5  # rows just past both launches' grid caps at D = 256 (8192 x 4 and 2048 x 16 rows)


@functools.lru_cache(maxsize=None)
def _rms_inputs(D, rows):
    """Small integers: |x|, |r| <= 2 so |s| <= 4, |gamma|, |dy| <= 2: sum s^2 <= 16 D and |sum g s| <= 16 D < 2^24."""
    x, r, dy = (integer_data((rows, D), "dense", seed=k).bfloat16().cuda() for k in (1, 2, 4))
    return x, r, integer_data((D,), "dense", seed=3).cuda(), dy, integer_data((rows, D), "sparse", seed=5).bfloat16().cuda()


@pytest.mark.parametrize("D,rows", list(itertools.product([256, 768, 2048, CROSS, 8192], [1, 5, 70])) + [(256, PAST_CAP)])
def test_rmsnorm_elementwise(D, rows):
    """ds: with t = rstd g (g one rounding, the product one), c = ((rstd rstd) rstd) ((sum g s) (1 / D)) (5 roundings with
    the rounded 1 / D; the sum is exact here), s c (one more) and the add and the subtraction (one each, of at most the
    sum of the magnitudes) the error is below 7 U (|ds_in| + |rstd g| + |s c|); 8 is used, doubled."""
    x, r, gamma, dy, dsi = _rms_inputs(D, rows)
    H, gd = hip(), gamma.double()
    y0, s0, rstd0 = H.rmsnorm_forward(x, None, gamma, EPS)
    assert s0.data_ptr() == x.data_ptr()
    ref = x.double() * rstd0.double()[:, None] * gd
    assert_rounds_from(y0, ref, 2.0 ** -22 * ref.abs(), "y without r")
    y, s, rstd = H.rmsnorm_forward(x, r, gamma, EPS)
    assert torch.equal(s, (x.float() + r.float()).bfloat16())
    sd, rs = s.double(), rstd.double()[:, None]
    want = torch.rsqrt(sd.pow(2).mean(1) + EPS)
    assert ((rstd.double() - want).abs() <= 8 * ulp_of(want, torch.float32)).all()
    ref = sd * rs * gd
    assert_rounds_from(y, ref, 2.0 ** -22 * ref.abs(), "y")
    g = dy.double() * gd
    c = rs ** 3 * (g * sd).sum(1, keepdim=True) / D
    terms = dy.double() * sd * rs
    for ds_in in (dsi, None):
        ds, dgamma = H.rmsnorm_backward(dy, ds_in, s, gamma, rstd)
        e = torch.zeros_like(sd) if ds_in is None else ds_in.double()
        assert_rounds_from(ds, e + rs * g - sd * c, 2 * 8 * U * (e.abs() + (rs * g).abs() + (sd * c).abs()), "ds")
        assert ((dgamma.double() - terms.sum(0)).abs() <= (rows + 4) * U * terms.abs().sum(0)).all()
        assert torch.equal(dgamma, H.rmsnorm_backward(dy, ds_in, s, gamma, rstd)[1])


@functools.lru_cache(maxsize=None)
def _glu_inputs(F, rows):
    """3 x randn gates and ups; in row 0 gates of +-30 and +-100, and ups of zero under two ordinary gates."""
    gen = torch.Generator().manual_seed(1000 * rows + F)
    gu = (torch.randn(rows, 2 * F, generator=gen) * 3).bfloat16()
    gu[0, :4] = torch.tensor([30.0, -30.0, 100.0, -100.0]).bfloat16()
    gu[0, F + 5:F + 7] = 0
    return gu.cuda(), torch.randn(rows, F, generator=gen).bfloat16().cuda()


def _glu_reference(gu, dh):
    """(h, dg, du) in float64 with their deltas: 6, 13 and 6 roundings (swiglu.hip's header), U each, doubled; dg's is
    taken from the magnitudes, because its factor 1 + g (1 - sg) crosses zero."""
    F = gu.shape[1] // 2
    g, u, d = gu[:, :F].double(), gu[:, F:].double(), dh.double()
    sg, om = torch.sigmoid(g), torch.sigmoid(-g)
    h, du = g * sg * u, d * g * sg
    return ((h, 12 * U * h.abs()), (d * u * sg * (1 + g * om), 26 * U * (d * u * sg).abs() * (1 + (g * om).abs())),
            (du, 12 * U * du.abs()))


@pytest.mark.parametrize("rows", [1, 3, 67])
@pytest.mark.parametrize("F", [8, 344, 11008])
def test_swiglu_elementwise(F, rows):
    gu, dh = _glu_inputs(F, rows)
    h, dgu = hip().swiglu_forward(gu), hip().swiglu_backward(dh, gu)
    assert h.shape == (rows, F) and dgu.shape == gu.shape
    (rh, eh), (rg, eg), (ru, eu) = _glu_reference(gu, dh)
    for name, got, ref, delta in (("h", h, rh, eh), ("dg", dgu[:, :F], rg, eg), ("du", dgu[:, F:], ru, eu)):
        assert torch.isfinite(got).all(), name
        assert_rounds_from(got.contiguous(), ref, delta, name)
    assert (dgu[:, :F][gu[:, F:] == 0] == 0).all() and (gu[:, F:] == 0).any()
    assert h[0, 2].item() == (gu[0, 2].float() * gu[0, F + 2].float()).bfloat16().item()  # g = +100: h = u g
    assert h[0, 3].item() == 0  # g = -100


def _grads(fn, inputs, gouts):
    leaves = [None if t is None else t.clone().requires_grad_(True) for t in inputs]
    outs = fn(*leaves)
    outs = outs if isinstance(outs, tuple) else (outs,)
    torch.autograd.backward(outs, gouts)
    return [o.detach() for o in outs], [None if t is None else t.grad for t in leaves]


def _near_bf16(a, b, mag):
    """Two bf16 roundings of one f32 value known to 64 U of its terms' magnitudes: one ulp at the larger."""
    a, b = a.double(), b.double()
    return ((a - b).abs() <= ulp_of(torch.maximum(a.abs(), b.abs()), torch.bfloat16) + 64 * U * mag).all()


def test_routes():
    """The ops take the fused path (bitwise the bindings' results) and stay within the composition's own bf16 error of
    it: y, h and the SwiGLU gradients are one rounding each way; the composition's ds rounds the norm's gradient and
    its sum with the skip gradient, the kernel rounds once: three bf16 roundings, 2^-8 each, of at most the sum of the
    magnitudes."""
    H = hip()
    x, r, gamma, dy, dsi = _rms_inputs(2048, 70)
    fn = lambda a, b, w: rn.add_rms_norm(a, b, w, EPS)
    (y, s), (dx, dr, dw) = _grads(fn, (x, r, gamma), (dy, dsi))
    by, bs, rstd = H.rmsnorm_forward(x, r, gamma, EPS)
    bds, bdg = H.rmsnorm_backward(dy, dsi, bs, gamma, rstd)
    assert all(torch.equal(a, b) for a, b in ((y, by), (s, bs), (dx, bds), (dr, bds), (dw, bdg)))
    gu, dh = _glu_inputs(344, 67)
    (h,), (dgu,) = _grads(sw.swiglu, (gu,), (dh,))
    assert torch.equal(h, H.swiglu_forward(gu)) and torch.equal(dgu, H.swiglu_backward(dh, gu))
    rn._ENABLED = sw._ENABLED = False
    try:
        (cy, cs), (cdx, cdr, cdw) = _grads(fn, (x, r, gamma), (dy, dsi))
        (ch,), (cdgu,) = _grads(sw.swiglu, (gu,), (dh,))
    finally:
        rn._ENABLED = sw._ENABLED = True
    sd, rs, g = s.double(), rstd.double()[:, None], dy.double() * gamma.double()
    mag = dsi.double().abs() + (rs * g).abs() + (sd * (rs ** 3 * (g * sd).sum(1, keepdim=True) / 2048)).abs()
    assert torch.equal(cs, s) and _near_bf16(cy, y, y.double().abs())
    assert ((cdx.double() - dx.double()).abs() <= 3 * 2.0 ** -8 * mag).all() and torch.equal(cdr, cdx)
    terms = (dy.double() * sd * rs).abs().sum(0)
    assert ((cdw.double() - dw.double()).abs() <= 2 * (70 + 4) * U * terms).all()
    (_, _), (_, eg), (_, eu) = _glu_reference(gu, dh)
    assert _near_bf16(ch, h, h.double().abs())
    assert _near_bf16(cdgu, dgu, torch.cat((eg, eu), 1) / U / 12)


def test_llama_model_against_f64():
    """Head dim 128 attention, rotary embeddings, grouped-query heads, both norms and SwiGLU in one model under bf16
    autocast: each parameter gradient within twice the error the torch compositions of the two ops show against float64
    in this same test.  The loss is one scalar, whose composition error can be small by chance: it also gets 2^-9, half
    a bf16 ulp of a logit of magnitude 1 (these logits stay below that), the rounding no path avoids."""
    kw = dict(d=256, layers=2, heads=2, kv_heads=1, ffn=344, vocab=128)
    torch.manual_seed(0)
    ref = get_model("llama", **kw).double()
    ids = synthetic_lm_batch(2, 64, 128, generator=torch.Generator().manual_seed(1))
    want = lm_loss(ref, ids)
    want.backward()

    def run(enabled):
        rn._ENABLED = sw._ENABLED = enabled
        try:
            m = get_model("llama", **kw)
            m.load_state_dict(ref.state_dict())
            m = m.float().cuda()
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = lm_loss(m, ids.cuda())
            loss.backward()
            return loss.item(), {n: p.grad for n, p in m.named_parameters()}
        finally:
            rn._ENABLED = sw._ENABLED = True

    (fl, fg), (cl, cg) = run(True), run(False)
    print("loss f64 %.6f fused %.6f composition %.6f" % (want.item(), fl, cl))
    assert abs(fl - want.item()) <= 2 * abs(cl - want.item()) + 2.0 ** -9
    for n, p in ref.named_parameters():
        ef, ec = rel_err(p.grad, fg[n].cpu()), rel_err(p.grad, cg[n].cpu())
        print("%-28s fused %.3e composition %.3e" % (n, ef, ec))
        assert ef <= 2 * ec, n


def _refusal_args():
    x, r, gamma, dy, dsi = _rms_inputs(256, 5)
    _, s, rstd = hip().rmsnorm_forward(x, r, gamma, EPS)
    odd = torch.zeros(5, 384, dtype=torch.bfloat16, device="cuda")
    fwd, bwd = [x, r, gamma, EPS], [dy, dsi, s, gamma, rstd]
    return {"rmsnorm_forward": fwd, "rmsnorm_backward": bwd, "x": x, "odd": odd, "gamma": gamma, "rstd": rstd}


@pytest.mark.parametrize("op,at,name,bad", [
    ("rmsnorm_forward", 0, "x", lambda a: a["x"].cpu()),
    ("rmsnorm_forward", 0, "x", lambda a: a["x"].float()),
    ("rmsnorm_forward", 0, "x", lambda a: a["x"][::2]),
    ("rmsnorm_forward", 0, "x", lambda a: a["odd"]),
    ("rmsnorm_forward", 1, "r", lambda a: a["x"][:2]),
    ("rmsnorm_forward", 1, "r", lambda a: a["x"].view(10, 128)),
    ("rmsnorm_forward", 2, "gamma", lambda a: a["gamma"][:128]),
    ("rmsnorm_forward", 2, "gamma", lambda a: a["gamma"].bfloat16()),
    ("rmsnorm_backward", 0, "dy", lambda a: a["odd"]),
    ("rmsnorm_backward", 0, "dy", lambda a: a["x"].cpu()),
    ("rmsnorm_backward", 1, "ds_in", lambda a: a["x"].view(10, 128)),
    ("rmsnorm_backward", 2, "s", lambda a: a["x"][:2]),
    ("rmsnorm_backward", 2, "s", lambda a: a["x"].float()),
    ("rmsnorm_backward", 3, "gamma", lambda a: a["gamma"][:128]),
    ("rmsnorm_backward", 4, "rstd", lambda a: a["rstd"][:3]),
    ("rmsnorm_backward", 4, "rstd", lambda a: a["rstd"].double()),
])
def test_rmsnorm_refusals(op, at, name, bad):
    a = _refusal_args()
    args = list(a[op])
    args[at] = bad(a)
    with pytest.raises(RuntimeError) as e:
        getattr(hip(), op)(*args)
    msg = str(e.value)
    assert msg.startswith(op + ": ") and (" " + name + " ") in msg, msg
