"""Argument checks of the kungfu_amd._hip bindings (csrc/kernels/bind_*.cpp, bind_util.hpp).

Table-driven: BASES holds one valid call per binding, at the smallest shape the exact / image-conv / stem suites
already run it at (no new shape reaches a kernel here); MUTATIONS changes one argument of a base call and the
binding has to refuse it, before it allocates or launches anything, with a RuntimeError that begins
"<binding>: " and names the argument.  The mutations are a CPU tensor in place of each secondary operand (the
device clause, on one GPU), a wrong dtype, NCHW-contiguous for channels_last, one channel too few, a statistics
workspace one element short, an `out` of the wrong shape, and a stride / padding of 2**31 (refused, not
truncated to 32 bits)."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8


@pytest.fixture(scope="module")
def H():
    from kungfu_amd._lib import hip

    return hip()


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _t(*shape, dtype=BF):
    t = torch.ones(*shape, dtype=dtype, device="cuda")
    return _cl(t) if t.dim() == 4 else t


def _stats(H, C, short=0):
    return torch.zeros(H.conv_stat_slots * 2 * C - short, dtype=torch.float64, device="cuda")


# ---- base calls: name -> (binding, H -> kwargs, shape of the (first) result) --------------------------------

def _conv(H):  # exact_cases.ROWS variant 24: 64 -> 64 channels, 3x3
    return dict(x=_t(3, 64, 9, 11), w=_t(64, 64, 3, 3), stride=1, variant=24)


def _conv_rect(H):  # exact_cases.RECT_IMAGE, RECT_CIN -> 32 channels, the 1x3 window
    return dict(x=_t(2, 128, 9, 11), w=_t(32, 128, 1, 3), stride=1, ph=0, pw=1)


def _dgrad_s2(H):  # exact_cases.S2_GRID, (Cout, Cin) = (64, 128)
    return dict(dy=_t(3, 64, 5, 6), wt=_t(128, 64, 3, 3), ks=3)


def _wgrad(H):  # exact_cases.WGRAD[1]
    return dict(dy=_t(2, 64, 7, 5), x=_t(2, 192, 7, 5), ks=3, stride=1)


def _gemm(H):  # exact_cases.GEMM[1]
    return dict(x=_t(70, 192), w=_t(256, 192))


def _gemm_nt(H):  # exact_cases.GEMM_NT_MN, K = 32
    return dict(a=_t(257, 32), b=_t(768, 32))


def _stem3_forward(H):  # exact_cases.STEM3[0], 32 channels
    return dict(x=_t(4, 3, 20, 18), wp=H.stem3_pack_weight(_t(32, 3, 2, 2)), kh=2, kw=2, stride=1, ph=0, pw=0)


def _stem3_wgrad(H):
    return dict(dy=_t(4, 32, 19, 17), x=_t(4, 3, 20, 18), kh=2, kw=2, stride=1, ph=0, pw=0)


def _stem_forward(H):  # exact_cases.STEM_IMAGES[1]
    return dict(x4=H.stem_pad4(_t(1, 3, 16, 9)), wp=H.stem_pack_weight(_t(64, 3, 7, 7)))


def _bn_forward(H):  # test_gpu.py::test_bn_backward_channel_slice_grad, C = 64
    return dict(x=_t(4, 64, 9, 11), res=None, weight=_t(64, dtype=F32), bias=_t(64, dtype=F32),
                running_mean=torch.zeros(64, device="cuda"), running_var=_t(64, dtype=F32), momentum=0.1, eps=1e-3,
                training=True, relu=True)


def _bn_backward(H):
    kw = _bn_forward(H)
    _, mean, invstd, coef, _ = H.bn_forward(**kw)
    return dict(dy=_t(4, 64, 9, 11), x=kw["x"], mean=mean, invstd=invstd, weight=kw["weight"], fcoef=coef, mask=None,
                relu=True, training=True, want_dres=False)


_STEM = {}


def _stem_chain(H):
    """The fused ResNet stem at test_gpu.py::test_stem_block_fused_backward_matches_fp32's (2, 37, 50) image:
    stem_forward -> bn_pool_forward -> bn_pool_backward(apply=False) -> stem_wgrad_bnp."""
    if not _STEM:
        torch.manual_seed(5)
        x4 = H.stem_pad4(_cl(torch.randn(2, 3, 37, 50, device="cuda").bfloat16()))
        st = _stats(H, 64)
        y = H.stem_forward(x4, H.stem_pack_weight(_cl((torch.randn(64, 3, 7, 7, device="cuda") * 0.1).bfloat16())), st)
        g = _t(64, dtype=F32)
        yp, mean, invstd, coef, arg, xarg = H.bn_pool_forward(y, g, torch.zeros(64, device="cuda"),
                                                              torch.zeros(64, device="cuda"), _t(64, dtype=F32), 0.1,
                                                              1e-5, True, None, st)
        _STEM["pool"] = dict(dy=torch.ones_like(yp), arg=arg, x=y, mean=mean, invstd=invstd, weight=g, fcoef=coef,
                             training=True, xarg=xarg, apply=False)
        bcoef = H.bn_pool_backward(**_STEM["pool"])[3]
        _STEM["bnp"] = dict(y=y, x4=x4, dyp=_STEM["pool"]["dy"], arg=arg, fcoef=coef, bcoef=bcoef)
    return _STEM


def _bn_pool_backward(H):
    return dict(_stem_chain(H)["pool"])


def _stem_wgrad_bnp(H):
    return dict(_stem_chain(H)["bnp"])


def _maxpool(H):  # test_gpu.py::test_maxpool2x2_gate_backward, C = 64
    return dict(x=_t(3, 64, 10, 12), dy=_t(3, 64, 5, 6), gate_stats=_stats(H, 64))


BASES = {
    "conv": ("conv", _conv, (3, 64, 9, 11)),
    "conv_rect": ("conv_rect", _conv_rect, (2, 32, 9, 11)),
    "conv_dgrad_s2": ("conv_dgrad_s2", _dgrad_s2, (3, 128, 10, 12)),
    "conv_wgrad": ("conv_wgrad", _wgrad, (64, 192, 3, 3)),
    "gemm": ("gemm", _gemm, (70, 256)),
    "gemm_nt": ("gemm_nt", _gemm_nt, (257, 768)),
    "stem3_forward": ("stem3_forward", _stem3_forward, (4, 32, 19, 17)),
    "stem3_wgrad": ("stem3_wgrad", _stem3_wgrad, (32, 3, 2, 2)),
    "stem_forward": ("stem_forward", _stem_forward, (1, 64, 8, 5)),
    "stem_wgrad_bnp": ("stem_wgrad_bnp", _stem_wgrad_bnp, (64, 3, 7, 7)),
    "bn_forward": ("bn_forward", _bn_forward, (4, 64, 9, 11)),
    "bn_backward": ("bn_backward", _bn_backward, (4, 64, 9, 11)),
    "bn_pool_backward": ("bn_pool_backward", _bn_pool_backward, (0,)),  # apply=False: no dx
    "maxpool2x2_backward": ("maxpool2x2_backward", _maxpool, (3, 64, 10, 12)),
}


@pytest.mark.parametrize("name", sorted(BASES))
def test_base_call_runs(H, name):
    """The table is not vacuous: every base call executes and returns the expected shape."""
    op, build, shape = BASES[name]
    out = getattr(H, op)(**build(H))
    out = out[0] if isinstance(out, (list, tuple)) else out
    torch.cuda.synchronize()
    assert tuple(out.shape) == shape


# ---- mutations ---------------------------------------------------------------------------------------------

def cpu(t):
    return t.cpu()


def f16(t):
    return t.to(torch.float16)


def nchw(t):
    assert t.dim() == 4 and not t.contiguous().is_contiguous(memory_format=torch.channels_last)
    return t.contiguous()


def less_ch(t):  # one channel (dim 1; the only dim of a vector) too few
    return _cl(t[:, :-1]) if t.dim() == 4 else t[..., :-1].contiguous()


def short(t):  # one element short
    return t.reshape(-1)[:-1].contiguous()


def strided(t):
    return torch.cat([t.reshape(-1), t.reshape(-1)])[::2]


def wider(t):  # an `out` of the wrong shape: one more column
    return _cl(torch.cat([t, t[..., :1]], -1)) if t.dim() == 4 else torch.cat([t, t[..., :1]], -1).contiguous()


# (base, argument the message has to name, kwargs -> changed kwargs)
def M(base, arg, fn=None, **add):
    """Mutate argument `arg` of the base call with fn, after adding the (valid) arguments `add` (callables of
    (H, kw) are evaluated against the base call)."""
    return (base, arg, fn, add)


def _like_out(name):
    return lambda H, kw: torch.zeros(BASES[name][2], dtype=BF, device="cuda").contiguous(
        memory_format=torch.channels_last if len(BASES[name][2]) == 4 else torch.contiguous_format)


def _st(C):
    return lambda H, kw: _stats(H, C)


def _vec(n, dtype=F32):
    return lambda H, kw: torch.ones(n, dtype=dtype, device="cuda")


_CONV_Y, _DX = _like_out("conv"), _like_out("conv_dgrad_s2")
_CONV_BWD = dict(stats=_st(64), bn_x=_CONV_Y)
_DG_BWD = dict(stats=_st(128), bn_x=_DX)
_RECT_BWD = dict(stats=_st(32), bn_x=_like_out("conv_rect"))

MUTATIONS = [
    # conv
    M("conv", "w", cpu), M("conv", "w", f16), M("conv", "w", nchw), M("conv", "x", nchw), M("conv", "w", less_ch),
    M("conv", "stats", short, stats=_st(64)), M("conv", "stats", cpu, stats=_st(64)),
    M("conv", "out", wider, out=_CONV_Y), M("conv", "out", cpu, out=_CONV_Y), M("conv", "out", nchw, out=_CONV_Y),
    M("conv", "bias", cpu, bias=_vec(64, BF)), M("conv", "bias", less_ch, bias=_vec(64, BF)),
    M("conv", "bias", lambda t: t.float(), bias=_vec(64, BF)),
    M("conv", "bn_x", cpu, **_CONV_BWD, bn_fcoef=_vec(128)), M("conv", "bn_x", less_ch, **_CONV_BWD, bn_fcoef=_vec(128)),
    M("conv", "bn_fcoef", cpu, **_CONV_BWD, bn_fcoef=_vec(128)),
    M("conv", "bn_fcoef", short, **_CONV_BWD, bn_fcoef=_vec(128)),
    M("conv", "bn_mask", cpu, **_CONV_BWD, bn_mask=_vec(3 * 64 * 9 * 11 // 8, U8)),
    M("conv", "bn_mask", short, **_CONV_BWD, bn_mask=_vec(3 * 64 * 9 * 11 // 8, U8)),
    M("conv", "acc_mask", cpu, out=_CONV_Y, acc_mask=_vec(3 * 64 * 9 * 11 // 8, U8)),
    M("conv", "stride", lambda s: 2 ** 31), M("conv", "variant", lambda v: 2 ** 31),
    # conv_rect (narrow: a stride or padding of 2**31 is refused, not truncated)
    M("conv_rect", "w", cpu), M("conv_rect", "w", nchw), M("conv_rect", "w", less_ch),
    M("conv_rect", "stats", short, stats=_st(32)), M("conv_rect", "out", wider, out=_like_out("conv_rect")),
    M("conv_rect", "bn_x", cpu, **_RECT_BWD, bn_fcoef=_vec(64)),
    M("conv_rect", "bn_fcoef", cpu, **_RECT_BWD, bn_fcoef=_vec(64)),
    M("conv_rect", "stride", lambda s: 2 ** 31), M("conv_rect", "ph", lambda p: 2 ** 31),
    M("conv_rect", "pw", lambda p: 2 ** 31),
    # conv_dgrad_s2 (bn_mask on the CPU: checked by conv, not by conv_dgrad_s2, before the checks were shared)
    M("conv_dgrad_s2", "wt", cpu), M("conv_dgrad_s2", "wt", nchw), M("conv_dgrad_s2", "dy", nchw),
    M("conv_dgrad_s2", "wt", less_ch),
    M("conv_dgrad_s2", "stats", short, **_DG_BWD, bn_fcoef=_vec(256)),
    M("conv_dgrad_s2", "bn_x", cpu, **_DG_BWD, bn_fcoef=_vec(256)),
    M("conv_dgrad_s2", "bn_fcoef", cpu, **_DG_BWD, bn_fcoef=_vec(256)),
    M("conv_dgrad_s2", "bn_mask", cpu, **_DG_BWD, bn_mask=_vec(3 * 128 * 10 * 12 // 8, U8)),
    M("conv_dgrad_s2", "bn_mask", short, **_DG_BWD, bn_mask=_vec(3 * 128 * 10 * 12 // 8, U8)),
    # conv_wgrad
    M("conv_wgrad", "dy", cpu), M("conv_wgrad", "dy", nchw), M("conv_wgrad", "dy", f16), M("conv_wgrad", "dy", wider),
    M("conv_wgrad", "out", wider, out=_like_out("conv_wgrad")), M("conv_wgrad", "out", cpu, out=_like_out("conv_wgrad")),
    M("conv_wgrad", "stride", lambda s: 2 ** 31),
    # gemm
    M("gemm", "w", cpu), M("gemm", "w", f16), M("gemm", "w", less_ch), M("gemm", "bias", cpu, bias=_vec(256, BF)),
    M("gemm", "bias", short, bias=_vec(256, BF)), M("gemm", "out", wider, out=_like_out("gemm")),
    M("gemm", "out", cpu, out=_like_out("gemm")),
    M("gemm", "gelu_u", cpu, gelu_u=_like_out("gemm"), stats=_st(256)),
    M("gemm", "stats", short, gelu_u=_like_out("gemm"), stats=_st(256)),
    # gemm_nt
    M("gemm_nt", "b", cpu), M("gemm_nt", "b", f16), M("gemm_nt", "b", less_ch),
    M("gemm_nt", "bias", cpu, bias=_vec(768, BF)), M("gemm_nt", "bias", short, bias=_vec(768, BF)),
    M("gemm_nt", "out", cpu, out=_like_out("gemm_nt")), M("gemm_nt", "out", short, out=_like_out("gemm_nt")),
    # stem3
    M("stem3_forward", "wp", cpu), M("stem3_forward", "wp", f16), M("stem3_forward", "x", nchw),
    M("stem3_forward", "bias", cpu, bias=_vec(32)), M("stem3_forward", "bias", f16, bias=_vec(32)),
    M("stem3_forward", "bias", short, bias=_vec(32)), M("stem3_forward", "stats", short, stats=_st(32)),
    M("stem3_forward", "stats", cpu, stats=_st(32)),
    M("stem3_forward", "out", wider, out=_like_out("stem3_forward")),
    M("stem3_forward", "out", nchw, out=_like_out("stem3_forward")),
    M("stem3_forward", "stride", lambda s: 2 ** 31), M("stem3_forward", "ph", lambda p: 2 ** 31),
    M("stem3_forward", "pw", lambda p: 2 ** 31),
    M("stem3_wgrad", "dy", cpu), M("stem3_wgrad", "dy", nchw), M("stem3_wgrad", "dy", wider),
    M("stem3_wgrad", "out", wider, out=_like_out("stem3_wgrad")), M("stem3_wgrad", "stride", lambda s: 2 ** 31),
    # the 7x7 stem (stem_wgrad_bnp checked neither the device of fcoef / bcoef / arg nor arg's contiguity)
    M("stem_forward", "wp", cpu), M("stem_forward", "wp", short), M("stem_forward", "stats", short, stats=_st(64)),
    M("stem_forward", "stats", cpu, stats=_st(64)), M("stem_forward", "x4", nchw),
    M("stem_wgrad_bnp", "y", cpu), M("stem_wgrad_bnp", "y", nchw), M("stem_wgrad_bnp", "dyp", cpu),
    M("stem_wgrad_bnp", "arg", cpu), M("stem_wgrad_bnp", "arg", strided), M("stem_wgrad_bnp", "arg", short),
    M("stem_wgrad_bnp", "fcoef", cpu), M("stem_wgrad_bnp", "fcoef", short), M("stem_wgrad_bnp", "bcoef", cpu),
    M("stem_wgrad_bnp", "bcoef", short),
    # BN (weight / bias were checked for dtype and size, not for the device)
    M("bn_forward", "weight", cpu), M("bn_forward", "bias", cpu), M("bn_forward", "weight", short),
    M("bn_forward", "weight", f16), M("bn_forward", "x", nchw), M("bn_forward", "res", nchw, res=_like_out("bn_forward")),
    M("bn_forward", "res", cpu, res=_like_out("bn_forward")), M("bn_forward", "sums", short, sums=_st(64)),
    M("bn_forward", "sums", cpu, sums=_st(64)),
    M("bn_backward", "dy", cpu), M("bn_backward", "dy", less_ch), M("bn_backward", "mean", cpu),
    M("bn_backward", "invstd", short), M("bn_backward", "weight", cpu), M("bn_backward", "fcoef", short),
    M("bn_backward", "fcoef", cpu), M("bn_backward", "sums", short, sums=_st(64)),
    M("bn_backward", "mask", cpu, mask=_vec(4 * 64 * 9 * 11 // 8, U8)),
    # bn_pool_backward passed mean / invstd / weight to the launcher unchecked, fcoef / arg / dy without a device
    M("bn_pool_backward", "mean", cpu), M("bn_pool_backward", "mean", short), M("bn_pool_backward", "invstd", cpu),
    M("bn_pool_backward", "invstd", short), M("bn_pool_backward", "weight", cpu), M("bn_pool_backward", "weight", short),
    M("bn_pool_backward", "fcoef", cpu), M("bn_pool_backward", "fcoef", short), M("bn_pool_backward", "arg", cpu),
    M("bn_pool_backward", "arg", short), M("bn_pool_backward", "dy", cpu), M("bn_pool_backward", "xarg", cpu),
    # pools
    M("maxpool2x2_backward", "dy", cpu), M("maxpool2x2_backward", "dy", nchw), M("maxpool2x2_backward", "dy", less_ch),
    M("maxpool2x2_backward", "gate_stats", short), M("maxpool2x2_backward", "gate_stats", cpu),
]


def _id(m):
    base, arg, fn, add = m
    return "%s-%s-%s" % (base, arg, getattr(fn, "__name__", "v").replace("<lambda>", "big"))


@pytest.mark.parametrize("mutation", MUTATIONS, ids=[_id(m) for m in MUTATIONS])
def test_mutation_is_refused(H, mutation):
    base, arg, fn, add = mutation
    op, build, _ = BASES[base]
    kw = build(H)
    kw.update({k: v(H, kw) for k, v in add.items()})
    kw[arg] = fn(kw[arg])
    with pytest.raises(RuntimeError) as e:
        getattr(H, op)(**kw)
    msg = str(e.value)
    assert msg.startswith(op + ": ") and re.search(r"\b%s\b" % re.escape(arg), msg.split("\n")[0][len(op) + 2:]), msg


def test_added_arguments_are_valid(H):
    """The arguments a mutation adds are themselves accepted: the conv BN-backward epilogue, its mask form and the
    stride-2 data gradient's run with them unmutated (shapes of test_gpu_exact.py's epilogue / dgrad cases)."""
    kw = _dgrad_s2(H)
    kw.update({k: v(H, kw) for k, v in dict(_DG_BWD, bn_fcoef=_vec(256)).items()})
    assert tuple(H.conv_dgrad_s2(**kw).shape) == BASES["conv_dgrad_s2"][2]
    kw = _conv_rect(H)
    kw.update({k: v(H, kw) for k, v in dict(_RECT_BWD, bn_fcoef=_vec(64)).items()})
    assert tuple(H.conv_rect(**kw).shape) == BASES["conv_rect"][2]
    torch.cuda.synchronize()


def test_conv3x3_aliases_are_gone(H):
    for name in ("conv3x3", "conv3x3_flip_weight", "conv3x3_supported", "conv3x3_variants"):
        assert not hasattr(H, name), name
    assert H.conv_variants() == 12
    assert H.conv_supported(64, 64, 3, 1) and not H.conv_supported(64, 64, 5, 1)
