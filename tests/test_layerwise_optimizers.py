"""CPU tests of the layer-wise optimizers (kungfu_amd/optimizers/layerwise.py): the plain LARS /
LAMB against a float64 transcription of their definitions, the zero-norm rules, the no-adaptation
group, the torch-op path of the fused classes over a FlatParamSpace, make_fused's routing, the
state_dict round trip and the chunk map."""
import copy
import itertools

import pytest
import torch

from kungfu_amd.optimizers import LAMB, LARS, FusedLAMB, FusedLARS
from kungfu_amd.optimizers.core import make_fused
from kungfu_amd.optimizers.layerwise import chunk_map, slot_offsets
from kungfu_amd.parallel.flat import FlatParamSpace

SHAPES = [(5, 3), (7,), (2, 3, 2)]


def _tensors(seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) * scale for s in SHAPES]


def _params(ts):
    return [torch.nn.Parameter(t.clone()) for t in ts]


# float64 transcriptions of the definitions (per tensor; python floats for every scalar)
def _lars64(w, g, m, lr, mu, wd, tc, eps, nesterov, trust=True):
    wn, gn = w.norm().item(), g.norm().item()
    q = tc * wn / (gn + wd * wn + eps) if (trust and wn > 0 and gn > 0) else 1.0
    d = q * (g + wd * w)
    m.mul_(mu).add_(d)
    w.sub_(lr * (d + mu * m if nesterov else m))
    return q


def _lamb64(w, g, m, v, t, lr, b1, b2, eps, wd, bias_correction, clip=1.0, trust=True):
    g = g * clip
    m.mul_(b1).add_((1 - b1) * g)
    v.mul_(b2).add_((1 - b2) * g * g)
    mh = m / (1 - b1 ** t) if bias_correction else m
    vh = v / (1 - b2 ** t) if bias_correction else v
    u = mh / (vh.sqrt() + eps) + wd * w
    wn, un = w.norm().item(), u.norm().item()
    r = wn / un if (trust and wn > 0 and un > 0) else 1.0
    w.sub_(lr * r * u)
    return r


@pytest.mark.parametrize("nesterov,momentum", itertools.product([False, True], [0.0, 0.9]))
def test_lars_equals_float64_transcription(nesterov, momentum):
    lr, wd, tc, eps = 0.1, 1e-2, 0.02, 1e-8
    ps = _params(_tensors(0))
    opt = LARS(ps, lr=lr, momentum=momentum, weight_decay=wd, trust_coefficient=tc, eps=eps, nesterov=nesterov)
    w64 = [p.detach().double() for p in ps]
    m64 = [torch.zeros_like(w) for w in w64]
    for s in range(3):
        gs = _tensors(10 + s, 0.1)
        for p, g, w, m in zip(ps, gs, w64, m64):
            p.grad = g.clone()
            _lars64(w, g.double(), m, lr, momentum, wd, tc, eps, nesterov)
        opt.step()
    for p, w in zip(ps, w64):
        torch.testing.assert_close(p.detach().double(), w, rtol=1e-6, atol=1e-7)  # a few f32 ulp over 3 steps


@pytest.mark.parametrize("bias_correction,max_grad_norm", itertools.product([True, False], [None, 100.0, 0.05]))
def test_lamb_equals_float64_transcription(bias_correction, max_grad_norm):
    """max_grad_norm 100 does not bind (the gradient's norm is about 0.5), 0.05 does."""
    lr, (b1, b2), eps, wd = 1e-2, (0.9, 0.999), 1e-6, 1e-2
    ps = _params(_tensors(0))
    opt = LAMB(ps, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, bias_correction=bias_correction,
               max_grad_norm=max_grad_norm)
    w64 = [p.detach().double() for p in ps]
    m64 = [torch.zeros_like(w) for w in w64]
    v64 = [torch.zeros_like(w) for w in w64]
    for s in range(3):
        gs = _tensors(10 + s, 0.1)
        tot = sum(g.double().square().sum().item() for g in gs) ** 0.5
        clip = 1.0 if max_grad_norm is None else min(1.0, max_grad_norm / tot)
        assert (clip < 1.0) == (max_grad_norm == 0.05)
        for p, g, w, m, v in zip(ps, gs, w64, m64, v64):
            p.grad = g.clone()
            _lamb64(w, g.double(), m, v, s + 1, lr, b1, b2, eps, wd, bias_correction, clip)
        opt.step()
    for p, w in zip(ps, w64):
        torch.testing.assert_close(p.detach().double(), w, rtol=1e-6, atol=1e-7)  # a few f32 ulp over 3 steps


@pytest.mark.parametrize("kind", ["lars", "lamb"])
@pytest.mark.parametrize("zero", ["weight", "grad"])
def test_zero_norm_gives_ratio_one_and_a_finite_update(kind, zero):
    """Through the fused classes' torch-op path, which records the ratios: an all-zero weight tensor
    and an all-zero gradient (for LAMB without decay, so that u is zero too) each get ratio 1 and
    the weights of the ratio-1 update."""
    lr, wd = 0.1, 0.1 if kind == "lars" else 0.0
    m = torch.nn.Linear(6, 4)
    if zero == "weight":
        with torch.no_grad():
            m.weight.zero_()
    w0 = m.weight.detach().clone()
    sp = FlatParamSpace(m.parameters(), reverse=False)
    opt = (FusedLARS(sp, lr=lr, momentum=0.0, weight_decay=wd, trust_coefficient=0.02) if kind == "lars"
           else FusedLAMB(sp, lr=lr, weight_decay=wd, bias_correction=False, eps=1e-6))
    g = torch.zeros(4, 6) if zero == "grad" else torch.randn(4, 6)
    sp.grad_view(0).copy_(g)
    sp.grad_view(1).copy_(torch.randn(4))
    opt.step()
    wn, xn, ratio = opt.trust_ratios()
    assert ratio[0].item() == 1.0 and ratio[1].item() != 1.0
    assert (wn[0].item() == 0.0) == (zero == "weight") and (xn[0].item() == 0.0) == (zero == "grad")
    assert torch.isfinite(sp.flat_param).all()
    if kind == "lars":
        want = w0 - lr * (g + wd * w0)
    else:  # m = 0.1 g, v = 0.001 g^2
        want = w0 - lr * (0.1 * g) / ((0.001 * g * g).sqrt() + 1e-6)
    torch.testing.assert_close(m.weight.detach(), want)


def test_no_trust_group_is_momentum_sgd():
    """trust=False, weight_decay=0: LARS moves the group exactly as torch's momentum SGD."""
    ts = _tensors(0)
    p1, p2 = _params(ts), _params(ts)
    o1 = LARS([dict(params=p1[:1]), dict(params=p1[1:], weight_decay=0.0, trust=False)], lr=0.1, momentum=0.9,
              weight_decay=1e-2)
    o2 = torch.optim.SGD(p2[1:], lr=0.1, momentum=0.9)
    for s in range(3):
        for a, b, g in zip(p1, p2, _tensors(10 + s, 0.1)):
            a.grad, b.grad = g.clone(), g.clone()
        o1.step()
        o2.step()
    for a, b in zip(p1[1:], p2[1:]):
        assert torch.equal(a, b)
    assert not torch.equal(p1[0], p2[0])


def test_no_trust_group_is_adam():
    """trust=False, weight_decay=0: LAMB is Adam with the same eps.  The two order their f32
    operations differently (torch folds the bias corrections into the step size), so "the same"
    is: equal to the float64 Adam recurrence as closely as torch's own Adam is (a few ulp), and
    within 1e-6 relative of torch's."""
    ts = _tensors(0)
    p1, p2 = _params(ts), _params(ts)
    o1 = LAMB([dict(params=p1[:1]), dict(params=p1[1:], weight_decay=0.0, trust=False)], lr=1e-2, eps=1e-6,
              weight_decay=1e-2)
    o2 = torch.optim.Adam(p2[1:], lr=1e-2, eps=1e-6)
    w64 = [t.double() for t in ts[1:]]
    m64 = [torch.zeros_like(w) for w in w64]
    v64 = [torch.zeros_like(w) for w in w64]
    for s in range(3):
        gs = _tensors(10 + s, 0.1)
        for a, b, g in zip(p1, p2, gs):
            a.grad, b.grad = g.clone(), g.clone()
        o1.step()
        o2.step()
        for w, m, v, g in zip(w64, m64, v64, gs[1:]):
            _lamb64(w, g.double(), m, v, s + 1, 1e-2, 0.9, 0.999, 1e-6, 0.0, True, trust=False)
    for a, b, w in zip(p1[1:], p2[1:], w64):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-7)
        e_lamb, e_adam = (a.detach().double() - w).abs().max(), (b.detach().double() - w).abs().max()
        assert e_lamb <= 2 * e_adam + 2.0 ** -24 * w.abs().max()


def _toy():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(37, 11), torch.nn.Tanh(), torch.nn.Linear(11, 3))


def _groups(m):
    return [dict(params=[p for p in m.parameters() if p.ndim > 1]),
            dict(params=[p for p in m.parameters() if p.ndim == 1], weight_decay=0.0, trust=False)]


def _padding(sp):
    mask = torch.ones(sp.numel, dtype=torch.bool)
    for o, n in sp.offsets:
        mask[o:o + n] = False
    return mask


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_fused_cpu_path_equals_plain(kind):
    """FusedLARS / FusedLAMB over a FlatParamSpace (torch ops on the CPU) against the plain optimizer
    on a copy of the model, at test_fused_adam_matches_torch's tolerance; the padding stays zero."""
    m1 = _toy()
    m2 = copy.deepcopy(m1)
    if kind == "lars":
        hp = dict(lr=0.1, momentum=0.9, weight_decay=1e-2, trust_coefficient=0.02, nesterov=True)
        o1 = LARS(_groups(m1), **hp)
    else:
        hp = dict(lr=1e-2, weight_decay=1e-2, max_grad_norm=1.0)
        o1 = LAMB(_groups(m1), **hp)
    sp = FlatParamSpace(m2.parameters())
    over = {p: dict(weight_decay=0.0, trust=False) for p in m2.parameters() if p.ndim == 1}
    o2 = (FusedLARS if kind == "lars" else FusedLAMB)(sp, overrides=over, **hp)
    for _ in range(4):
        x = torch.randn(8, 37)
        for m, o in [(m1, o1), (m2, o2)]:
            o.zero_grad()
            m(x).square().sum().backward()
            o.step()
    for a, b in zip(m1.parameters(), m2.parameters()):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)
    pad = _padding(sp)
    assert pad.any()
    for buf in [sp.flat_param] + [b for k, b in o2._flat_state().items() if k != "step" and b is not None]:
        assert not buf[pad].any()
    wn, xn, ratio = o2.trust_ratios()
    for k, p in enumerate(sp.params):
        assert (ratio[k].item() == 1.0) == (p.ndim == 1)


@pytest.mark.parametrize("cls", [LARS, LAMB])
def test_make_fused_routes_one_and_two_groups(cls):
    fused = FusedLARS if cls is LARS else FusedLAMB
    m = _toy()
    sp = FlatParamSpace(m.parameters())
    one = make_fused(cls(m.parameters(), lr=0.05, weight_decay=0.02), sp)
    assert type(one) is fused and len(one.param_groups) == 1 and one.param_groups[0]["lr"] == 0.05
    assert one.wd_tab.tolist() == pytest.approx([0.02] * 4) and one.trust_tab.tolist() == [1.0] * 4
    two = make_fused(cls(_groups(m), lr=0.05, weight_decay=0.02), sp)
    assert type(two) is fused and len(two.param_groups) == 1
    for k, p in enumerate(sp.params):
        assert two.wd_tab[k].item() == pytest.approx(0.0 if p.ndim == 1 else 0.02)
        assert two.trust_tab[k].item() == (0.0 if p.ndim == 1 else 1.0)


def test_make_fused_refuses_groups_that_differ_elsewhere():
    m = _toy()
    sp = FlatParamSpace(m.parameters())
    gs = _groups(m)
    gs[1]["lr"] = 0.5
    assert make_fused(LARS(gs, lr=0.05), sp) is None
    assert make_fused(LAMB(gs, lr=0.05), sp) is None
    gs = _groups(m)
    gs[1]["betas"] = (0.8, 0.99)
    assert make_fused(LAMB(gs, lr=0.05), sp) is None
    gs = _groups(m)
    gs[1]["momentum"] = 0.5
    assert make_fused(LARS(gs, lr=0.05), sp) is None
    # the single-group rule of the existing routes is untouched
    assert make_fused(torch.optim.SGD([dict(params=g["params"]) for g in _groups(m)], lr=0.1), sp) is None
    assert make_fused(torch.optim.SGD(m.parameters(), lr=0.1), sp) is not None


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_state_dict_round_trip(kind):
    def build():
        m = _toy()
        sp = FlatParamSpace(m.parameters())
        opt = FusedLARS(sp, lr=0.1, weight_decay=1e-2) if kind == "lars" else FusedLAMB(sp, lr=1e-2, weight_decay=1e-2)
        return m, sp, opt

    def train(m, opt, xs):
        for x in xs:
            opt.zero_grad()
            m(x).square().sum().backward()
            opt.step()

    xs = [torch.randn(8, 37) for _ in range(4)]
    m1, sp1, o1 = build()
    train(m1, o1, xs[:2])
    sd = copy.deepcopy(o1.state_dict())
    assert set(sd["kungfu_flat"]) == ({"momentum_buffer"} if kind == "lars" else {"exp_avg", "exp_avg_sq", "step"})
    m2, sp2, o2 = build()
    m2.load_state_dict(m1.state_dict())
    o2.load_state_dict(sd)
    for a, b in zip(o1._flat_state().values(), o2._flat_state().values()):
        assert torch.equal(a, b)
    train(m1, o1, xs[2:])
    train(m2, o2, xs[2:])
    assert torch.equal(sp1.flat_param, sp2.flat_param)


@pytest.mark.parametrize("chunk", [64, 256, 4096])
def test_chunk_map_covers_every_slot_once(chunk):
    sizes = [1, 63, 64, 65, chunk - 64 or 64, chunk, chunk + 64, 3 * chunk + 1]
    sp = FlatParamSpace([torch.nn.Parameter(torch.zeros(n)) for n in sizes], reverse=False)
    offs = slot_offsets(sp)
    assert offs[0] == 0 and offs[-1] == sp.numel and all(o % 64 == 0 for o in offs)
    chunks, first = chunk_map(offs, chunk)
    assert first[0].item() == 0 and first[-1].item() == chunks.shape[0] and len(first) == len(sizes) + 1
    hits = torch.zeros(sp.numel, dtype=torch.int32)
    for c, (start, slot, length) in enumerate(chunks.tolist()):
        assert 0 < length <= chunk and start % 64 == 0 and length % 64 == 0
        assert offs[slot] <= start and start + length <= offs[slot + 1], "chunk %d crosses a slot boundary" % c
        assert first[slot].item() <= c < first[slot + 1].item()
        hits[start:start + length] += 1
    assert (hits == 1).all()
    with pytest.raises(ValueError):
        chunk_map([0, 128, 64], chunk)
