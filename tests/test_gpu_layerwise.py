"""GPU tests of the fused LARS / LAMB kernels (csrc/kernels/layerwise.hip) and their routing.

Slot sizes sit around the chunk size C the extension exports (1, 63, 64, 65, C - 64, C, C + 64,
3 C + 1) and one case has more chunks than the exported grid cap.  The float64 references below are
transcriptions of the definitions in kungfu_amd/optimizers/layerwise.py, started from the same f32
inputs; the plain f32 optimizers run on the GPU in torch ops.
"""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")


@pytest.fixture(scope="module")
def H():
    from kungfu_amd._lib import hip

    return hip()


def _sizes(H):
    C = H.layerwise_chunk
    return [1, 63, 64, 65, C - 64, C, C + 64, 3 * C + 1]


def _space(tensors):
    from kungfu_amd.parallel.flat import FlatParamSpace

    ps = [torch.nn.Parameter(t.clone().cuda()) for t in tensors]
    return FlatParamSpace(ps, reverse=False), ps


def _set_grads(sp, grads):
    sp.flat_grad.zero_()
    for i, g in enumerate(grads):
        sp.grad_view(i).copy_(g)


def _randn_list(sizes, seed, scale):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) * scale for n in sizes]


def _ulp32(x64):
    """One f32 ulp at |x| (x: f64 tensor), as f64."""
    a = x64.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def _padding_mask(sp):
    m = torch.ones(sp.numel, dtype=torch.bool, device=sp.device)
    for o, n in sp.offsets:
        m[o:o + n] = False
    return m


# -- float64 transcriptions of the definitions -------------------------------------------------------------

def _ref_lars(ws, gs, ms, lr, mu, wds, trusts, tc, eps, nesterov):
    for w, g, m, wd, tr in zip(ws, gs, ms, wds, trusts):
        wn, gn = w.norm().item(), g.norm().item()
        q = tc * wn / (gn + wd * wn + eps) if (tr and wn > 0 and gn > 0) else 1.0
        d = q * (g + wd * w)
        m.mul_(mu).add_(d)
        w.sub_(lr * (d + mu * m if nesterov else m))


def _ref_lamb(ws, gs, ms, vs, t, lr, b1, b2, eps, wds, trusts, bias_correction, max_grad_norm):
    clip = 1.0
    if max_grad_norm is not None:
        tot = sum(g.square().sum().item() for g in gs) ** 0.5
        clip = min(1.0, max_grad_norm / tot) if tot > 0 else 1.0
    for w, g, m, v, wd, tr in zip(ws, gs, ms, vs, wds, trusts):
        g = g * clip
        m.mul_(b1).add_((1 - b1) * g)
        v.mul_(b2).add_((1 - b2) * g * g)
        mh = m / (1 - b1 ** t) if bias_correction else m
        vh = v / (1 - b2 ** t) if bias_correction else v
        u = mh / (vh.sqrt() + eps) + wd * w
        wn, un = w.norm().item(), u.norm().item()
        r = wn / un if (tr and wn > 0 and un > 0) else 1.0
        w.sub_(lr * r * u)


# -- norms -------------------------------------------------------------------------------------------------

def _check_norm(norm32, sumsq64, what):
    """sumsq64 lies within one f32 ulp of the returned norm: (n - ulp)^2 <= S <= (n + ulp)^2."""
    n = norm32.double()
    u = _ulp32(n)
    lo, hi = (n - u).clamp(min=0).square(), (n + u).square()
    ok = (sumsq64 >= lo) & (sumsq64 <= hi)
    assert ok.all(), "%s: norms %s vs sqrt of f64 sums %s" % (what, n.tolist(), sumsq64.sqrt().tolist())


@needs_gpu
@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_norms_exact_on_integer_data(H, kind):
    """Small-integer w and g (|.| <= 2, at most 3C + 1 elements per slot: every sum < 2^24): the
    per-slot ||w|| (both optimizers) and LARS's ||g|| are the f32 roundings of the exact sums; an
    all-zero weight slot and a zero-gradient slot get ratio 1."""
    from kungfu_amd.optimizers import FusedLAMB, FusedLARS
    from kungfu_amd.utils.numerics import integer_data

    sizes = _sizes(H) + [64, 65]
    ws = [integer_data((n,), "dense", seed=10 + i) for i, n in enumerate(sizes)]
    gs = [integer_data((n,), "dense", seed=50 + i) for i, n in enumerate(sizes)]
    ws[-2].zero_()
    gs[-1].zero_()
    sp, _ = _space(ws)
    _set_grads(sp, gs)
    opt = FusedLARS(sp, lr=0.0, weight_decay=0.5) if kind == "lars" else FusedLAMB(sp, lr=0.0, weight_decay=0.0)
    opt.step()
    wn, xn, ratio = opt.trust_ratios()
    sw = torch.stack([w.double().square().sum() for w in ws]).cuda()
    _check_norm(wn, sw, "w_norm")
    assert ratio[-2].item() == 1.0
    if kind == "lars":
        sg = torch.stack([g.double().square().sum() for g in gs]).cuda()
        _check_norm(xn, sg, "x_norm")
        assert ratio[-1].item() == 1.0 and xn[-1].item() == 0.0
        assert (ratio[:-2] != 1.0).all()
    assert wn[-2].item() == 0.0
    assert torch.isfinite(sp.flat_param).all()


@needs_gpu
def test_more_chunks_than_the_grid_cap(H):
    """One slot of (cap + 1) C elements in {-1, 0, 1}: the chunk loop runs twice for block 0; the
    norms are exact and every element, the last chunk's included, gets the LARS update."""
    from kungfu_amd.optimizers import FusedLARS
    from kungfu_amd.utils.numerics import integer_data

    n = (H.layerwise_grid_cap + 1) * H.layerwise_chunk
    w0, g0 = integer_data((n,), "sparse", seed=1), integer_data((n,), "sparse", seed=2)
    sp, _ = _space([w0])
    _set_grads(sp, [g0])
    lr, wd, tc, eps = 0.5, 0.25, 0.02, 1e-8
    opt = FusedLARS(sp, lr=lr, momentum=0.0, weight_decay=wd, trust_coefficient=tc, eps=eps)
    opt.step()
    wn, xn, ratio = opt.trust_ratios()
    w64, g64 = w0.double().cuda(), g0.double().cuda()
    _check_norm(wn, w64.square().sum().reshape(1), "w_norm")
    _check_norm(xn, g64.square().sum().reshape(1), "x_norm")
    a, b = w64.norm().item(), g64.norm().item()
    q = tc * a / (b + wd * a + eps)
    assert abs(ratio.item() / q - 1) < 1e-6
    ref = w64 - lr * q * (g64 + wd * w64)
    torch.testing.assert_close(sp.flat_param.double(), ref, rtol=1e-6, atol=1e-7)


@needs_gpu
def test_lamb_update_norm(H):
    """||u|| per slot against float64 computed from the kernel's own updated m, v: relative error
    below 1e-5 (test_norms_variance_axpby's bound for sumsq2)."""
    from kungfu_amd.optimizers import FusedLAMB

    sizes = _sizes(H)
    sp, _ = _space(_randn_list(sizes, 3, 0.5))
    lr, (b1, b2), eps, wd = 0.0, (0.9, 0.999), 1e-6, 0.01
    opt = FusedLAMB(sp, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    for t in (1, 2):
        _set_grads(sp, _randn_list(sizes, 20 + t, 0.1))
        opt.step()
        m, v, w = opt.exp_avg.double(), opt.exp_avg_sq.double(), sp.flat_param.double()
        u = (m / (1 - b1 ** t)) / ((v / (1 - b2 ** t)).sqrt() + eps) + wd * w
        xn = opt.trust_ratios()[1].double()
        for k, (o, n) in enumerate(sp.offsets):
            ref = u[o:o + n].norm().item()
            assert abs(xn[k].item() / ref - 1) < 1e-5, (t, k, xn[k].item(), ref)


# -- element-wise against float64 --------------------------------------------------------------------------

_NO_ADAPT = (3, 6)  # slots (65 and C + 64 elements) with weight_decay 0 and trust off


@functools.lru_cache(maxsize=None)
def _inputs(chunk, steps):
    C = chunk
    sizes = [1, 63, 64, 65, C - 64, C, C + 64, 3 * C + 1]
    return sizes, _randn_list(sizes, 7, 0.5), [_randn_list(sizes, 100 + s, 0.05) for s in range(steps)]


def _run_three_ways(kind, hp, steps, H):
    """(fused w, plain w, f64 w) per tensor after `steps` steps from the same f32 start."""
    from kungfu_amd.optimizers import LAMB, LARS, FusedLAMB, FusedLARS

    sizes, w0, grads = _inputs(H.layerwise_chunk, steps)
    sp, ps = _space(w0)
    over = {ps[k]: dict(weight_decay=0.0, trust=False) for k in _NO_ADAPT}
    qs = [torch.nn.Parameter(w.clone().cuda()) for w in w0]
    groups = [dict(params=[q for k, q in enumerate(qs) if k not in _NO_ADAPT]),
              dict(params=[qs[k] for k in _NO_ADAPT], weight_decay=0.0, trust=False)]
    if kind == "lars":
        fused, plain = FusedLARS(sp, overrides=over, **hp), LARS(groups, **hp)
    else:
        fused, plain = FusedLAMB(sp, overrides=over, **hp), LAMB(groups, **hp)
    w64 = [w.double().cuda() for w in w0]
    m64 = [torch.zeros_like(w) for w in w64]
    v64 = [torch.zeros_like(w) for w in w64]
    wds = [0.0 if k in _NO_ADAPT else hp["weight_decay"] for k in range(len(sizes))]
    trusts = [k not in _NO_ADAPT for k in range(len(sizes))]
    for s in range(steps):
        gs = [g.cuda() for g in grads[s]]
        _set_grads(sp, gs)
        for q, g in zip(qs, gs):
            q.grad = g.clone()
        fused.step()
        plain.step()
        g64 = [g.double() for g in gs]
        if kind == "lars":
            _ref_lars(w64, g64, m64, hp["lr"], hp["momentum"], wds, trusts, hp["trust_coefficient"], hp["eps"],
                      hp["nesterov"])
        else:
            _ref_lamb(w64, g64, m64, v64, s + 1, hp["lr"], hp["betas"][0], hp["betas"][1], hp["eps"], wds, trusts,
                      hp["bias_correction"], hp["max_grad_norm"])
    assert not sp.flat_param[_padding_mask(sp)].any(), "padding moved"
    return [sp.param_view(i).detach() for i in range(len(sizes))], [q.detach() for q in qs], w64


def _assert_within_4x_plain(kind, hp, steps, H):
    fw, pw, rw = _run_three_ways(kind, hp, steps, H)
    f = torch.cat([a.double() for a in fw])
    p = torch.cat([a.double() for a in pw])
    r = torch.cat(rw)
    assert torch.isfinite(f).all()
    err_f, err_p = (f - r).abs(), (p - r).abs()
    e_plain = err_p.max().item()
    excess = (err_f - _ulp32(r)).max().item()
    print("layerwise %s %s steps=%d: max err fused %.3e plain %.3e ratio %.3f" %
          (kind, {k: v for k, v in hp.items() if k not in ("lr", "eps")}, steps, err_f.max().item(), e_plain,
           err_f.max().item() / max(e_plain, 1e-300)))
    assert excess <= 4 * e_plain, (err_f.max().item(), e_plain)


@needs_gpu
@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("nesterov", [False, True])
def test_lars_against_float64(H, nesterov, momentum, steps):
    """Max error of the kernel <= 4 x the plain f32 optimizer's against the same float64 reference,
    plus one f32 ulp of |w| (summation order and the kernel's contracted multiply-adds differ)."""
    hp = dict(lr=0.1, momentum=momentum, weight_decay=1e-2, trust_coefficient=0.02, eps=1e-8, nesterov=nesterov)
    _assert_within_4x_plain("lars", hp, steps, H)


@needs_gpu
@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("max_grad_norm", [1e6, 1.0], ids=["clip_idle", "clip_binding"])
@pytest.mark.parametrize("bias_correction", [True, False])
def test_lamb_against_float64(H, bias_correction, max_grad_norm, steps):
    """As above for LAMB; the whole gradient's norm is about 9 here, so max_grad_norm = 1 binds."""
    hp = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-6, weight_decay=1e-2, bias_correction=bias_correction,
              max_grad_norm=max_grad_norm)
    _assert_within_4x_plain("lamb", hp, steps, H)


# -- isolation, determinism, side effects ------------------------------------------------------------------

def _make(kind, sp, **kw):
    from kungfu_amd.optimizers import FusedLAMB, FusedLARS

    if kind == "lars":
        return FusedLARS(sp, lr=0.1, momentum=0.9, weight_decay=1e-2, trust_coefficient=0.02, **kw)
    return FusedLAMB(sp, lr=1e-2, weight_decay=1e-2, **kw)


def _state(opt):
    bufs = [opt.space.flat_param] + [b for b in opt._flat_state().values() if b is not None]
    return [b.clone() for b in bufs]


def _two_steps(kind, sizes, changed=None):
    """Two steps from a fixed start; the second step's gradient of slot `changed` is another draw."""
    sp, _ = _space(_randn_list(sizes, 5, 0.5))
    opt = _make(kind, sp)
    for s in range(2):
        gs = _randn_list(sizes, 30 + s, 0.05)
        if s == 1 and changed is not None:
            gs[changed] = _randn_list(sizes, 99, 0.05)[changed]
        _set_grads(sp, gs)
        g0 = sp.flat_grad.clone()
        opt.step()
        assert torch.equal(sp.flat_grad, g0), "the step wrote flat_grad"
    return sp, _state(opt)


@needs_gpu
@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_slot_isolation_and_determinism(H, kind):
    """Changing one slot's gradient changes that slot's weights and state only, bit for bit, for a
    slot that ends exactly on a chunk boundary (C elements) and for its neighbour; equal inputs give
    equal bits; flat_grad is only read."""
    C = H.layerwise_chunk
    sizes = [65, C, C + 64, 2 * C, 63]
    sp, base = _two_steps(kind, sizes)
    _, again = _two_steps(kind, sizes)
    for a, b in zip(base, again):
        assert torch.equal(a, b), "two runs from equal state differ"
    offs = [o for o, _ in sp.offsets] + [sp.numel]
    for k in (1, 2):
        _, other = _two_steps(kind, sizes, changed=k)
        inside = torch.zeros(sp.numel, dtype=torch.bool, device="cuda")
        inside[offs[k]:offs[k + 1]] = True
        for a, b in zip(base, other):
            if a.numel() != sp.numel:  # the step count
                assert torch.equal(a, b)
                continue
            assert torch.equal(a[~inside], b[~inside]), "slot %d's gradient reached another slot" % k
            assert not torch.equal(a[inside], b[inside])
        assert not other[0][_padding_mask(sp)].any()


@needs_gpu
@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_shadow_written_with_the_weights(H, kind):
    sizes = _sizes(H)
    sp, _ = _space(_randn_list(sizes, 5, 0.5))
    sp.enable_shadow()
    opt = _make(kind, sp)
    _set_grads(sp, _randn_list(sizes, 31, 0.05))
    before = sp.flat_shadow.clone()
    opt.step()
    assert not torch.equal(before, sp.flat_shadow)
    assert torch.equal(sp.flat_shadow.view(torch.int16), sp.flat_param.bfloat16().view(torch.int16))


def _graph_shape(g):
    """(nodes, edges, roots) of a kept captured graph."""
    rt = ctypes.CDLL("libamdhip64.so")
    h = ctypes.c_void_p(g.raw_cuda_graph())
    out = []
    n = ctypes.c_size_t(0)
    assert rt.hipGraphGetNodes(h, None, ctypes.byref(n)) == 0
    out.append(n.value)
    n = ctypes.c_size_t(0)
    assert rt.hipGraphGetEdges(h, None, None, ctypes.byref(n)) == 0
    out.append(n.value)
    n = ctypes.c_size_t(0)
    assert rt.hipGraphGetRootNodes(h, None, ctypes.byref(n)) == 0
    out.append(n.value)
    return tuple(out)


@needs_gpu
@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_graph_replay_equals_eager(H, kind):
    """A captured step is one chain of nodes (no side stream) and, replayed after _lr_t and the
    gradient changed, equals the same eager step bit for bit."""
    sizes = _sizes(H)
    kw = dict(max_grad_norm=1.0) if kind == "lamb" else {}
    g1, g2 = _randn_list(sizes, 41, 0.05), _randn_list(sizes, 42, 0.05)

    def fresh():
        sp, _ = _space(_randn_list(sizes, 5, 0.5))
        opt = _make(kind, sp, **kw)
        _set_grads(sp, g1)
        opt.step()  # state and step count are non-trivial before the step under test
        return sp, opt

    sp_e, opt_e = fresh()
    _set_grads(sp_e, g2)
    opt_e.param_groups[0]["lr"] = 0.03
    opt_e.step()
    eager = _state(opt_e)

    sp_g, opt_g = fresh()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        opt_g.step()
    nodes, edges, roots = _graph_shape(graph)
    assert nodes >= 3 and roots == 1 and edges == nodes - 1, (nodes, edges, roots)
    graph.instantiate()
    _set_grads(sp_g, g2)
    opt_g._lr_t.fill_(0.03)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, _state(opt_g)):
        assert torch.equal(a, b)


# -- routing through the wrapper ---------------------------------------------------------------------------

def _train(models_opts, batches, loss):
    for x in batches:
        for m, o in models_opts:
            o.zero_grad()
            loss(m(x)).backward()
            o.step()


@needs_gpu
def test_wrapper_runs_fused_lars(H):
    """SynchronousSGDOptimizer(LARS(...)) on test_fused_sgd_matches_torch's conv + linear toy: the
    inner optimizer is a FusedLARS and three steps match plain LARS at that test's tolerance."""
    import kungfu_amd as kf
    from kungfu_amd.optimizers import LARS, FusedLARS

    kf.init()
    torch.manual_seed(0)

    def toy():
        return torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3), torch.nn.Flatten(), torch.nn.Linear(8 * 6 * 6, 5)).cuda()

    m1, m2, m3 = toy(), toy(), toy()
    m2.load_state_dict(m1.state_dict())
    m3.load_state_dict(m1.state_dict())
    m2 = m2.to(memory_format=torch.channels_last)

    def groups(m):
        return [dict(params=[p for p in m.parameters() if p.ndim > 1]),
                dict(params=[p for p in m.parameters() if p.ndim == 1], weight_decay=0.0, trust=False)]

    hp = dict(lr=0.1, momentum=0.9, weight_decay=1e-3, trust_coefficient=0.02)
    o1 = LARS(groups(m1), **hp)
    o2 = kf.optimizers.SynchronousSGDOptimizer(kf.optimizers.LARS(groups(m2), **hp))
    o3 = kf.optimizers.SynchronousSGDOptimizer(kf.optimizers.LARS(groups(m3), **hp), fused=False)
    assert isinstance(o2.inner, FusedLARS)
    assert type(o3.inner) is LARS
    k_bias = o2.space.index(m2[2].bias)
    assert o2.inner.trust_tab[k_bias].item() == 0.0 and o2.inner.wd_tab[k_bias].item() == 0.0
    _train([(m1, o1), (m2, o2), (m3, o3)], [torch.randn(4, 3, 8, 8, device="cuda") for _ in range(3)],
           lambda y: y.square().mean())
    for a, b, c in zip(m1.parameters(), m2.parameters(), m3.parameters()):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(a, c, rtol=1e-4, atol=1e-4)
    assert (o2.inner.trust_ratios()[2][k_bias] == 1.0).item()


@needs_gpu
def test_wrapper_runs_fused_lamb(H):
    """The same for LAMB on test_fused_adam_matches_torch's linear toy, at that test's tolerance."""
    import kungfu_amd as kf
    from kungfu_amd.optimizers import LAMB, FusedLAMB

    kf.init()
    torch.manual_seed(0)
    m1, m2, m3 = (torch.nn.Linear(37, 11).cuda() for _ in range(3))
    m2.load_state_dict(m1.state_dict())
    m3.load_state_dict(m1.state_dict())
    hp = dict(lr=1e-2, weight_decay=0.01, max_grad_norm=1.0)
    o1 = LAMB(m1.parameters(), **hp)
    o2 = kf.optimizers.SynchronousSGDOptimizer(kf.optimizers.LAMB(m2.parameters(), **hp))
    o3 = kf.optimizers.SynchronousSGDOptimizer(kf.optimizers.LAMB(m3.parameters(), **hp), fused=False)
    assert isinstance(o2.inner, FusedLAMB)
    assert type(o3.inner) is LAMB
    _train([(m1, o1), (m2, o2), (m3, o3)], [torch.randn(8, 37, device="cuda") for _ in range(3)],
           lambda y: y.square().sum())
    for a, b, c in zip(m1.parameters(), m2.parameters(), m3.parameters()):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(a, c, rtol=1e-4, atol=1e-5)


# -- binding refusals --------------------------------------------------------------------------------------

def _lars_args(H):
    from kungfu_amd.optimizers import FusedLARS

    sp, _ = _space(_randn_list([100, 64, 300], 5, 0.5))  # slots of 128, 64, 320 elements
    opt = FusedLARS(sp, lr=0.1)
    args = dict(w=sp.flat_param, g=sp.flat_grad, m=opt.momentum_buffer, shadow=None, offsets=opt._offsets,
                chunks=opt._chunks, slot_chunk0=opt._slot_chunk0, partials=opt._partials, wd_tab=opt.wd_tab,
                trust_tab=opt.trust_tab, w_norm=opt.w_norm, x_norm=opt.x_norm, ratio=opt.ratio, lr=0.1,
                lr_t=opt._lr_t, mu=0.9, tc=0.001, eps=1e-8, gscale=1.0, nesterov=False)
    return sp, opt, args


@needs_gpu
@pytest.mark.parametrize("step", ["lars_step", "lamb_step"])
@pytest.mark.parametrize("bad,named", [
    (dict(offsets=[0, 192, 128, 512]), "offsets"),   # not ascending
    (dict(offsets=[0, 100, 192, 512]), "offsets"),   # not a multiple of 64
    (dict(offsets=[0, 128, 192, 448]), "offsets"),   # does not end at numel
    (dict(wd_tab="cpu"), "wd_tab"),                  # a host table
    (dict(trust_tab="short"), "trust_tab"),          # a table one short
    (dict(ratio="short"), "ratio"),
])
def test_binding_refusals(H, step, bad, named):
    """Each refusal is a RuntimeError naming the argument, raised before anything is launched."""
    sp, opt, args = _lars_args(H)
    assert opt._offsets.tolist() == [0, 128, 192, 512]
    if step == "lamb_step":
        for k in ("mu", "tc", "nesterov"):
            args.pop(k)
        args.update(v=torch.zeros_like(sp.flat_param), b1=0.9, b2=0.999, step=torch.ones(1, device="cuda"),
                    bias_correction=True, eps=1e-6)
    getattr(H, step)(**args)  # the unmodified call is accepted
    for k, v in bad.items():
        if k == "offsets":
            args[k] = torch.tensor(v, dtype=torch.int64)
        elif v == "cpu":
            args[k] = args[k].cpu()
        else:
            args[k] = args[k][:-1].contiguous()
    torch.cuda.synchronize()
    w0 = sp.flat_param.clone()
    with pytest.raises(RuntimeError, match=r"%s: .*%s" % (step, named)):
        getattr(H, step)(**args)
    torch.cuda.synchronize()
    assert torch.equal(sp.flat_param, w0)
