"""Bit-exact tests of the MFMA conv / GEMM / stem kernels on integer data.

With small-integer bf16 operands every product and every f32 partial sum is an exact integer, so a
kernel's output equals the float64 torch reference of the same operation bit for bit whatever its
summation order, tile shape, split count or atomics: no tolerance, and one wrong element -- a pixel that
lost a tap at an image border, a wrong sub-tile corner, a dropped 8-channel chunk, a store past M, a wrong
rounding mode -- fails the test (tests/test_numerics_helper.py shows the 1e-2 criteria of the randn tests
accepting such errors).  Inputs and references come from tests/exact_cases.py, whose every recipe is
checked against its preconditions on the CPU; the reference is always torch in float64, never another
variant of the kernel.

Combinations that are not run.  A launcher may refuse a combination with an exception; every refusal must
match a row of REJECTIONS below (a refusal that is not listed, or a listed one that runs, fails the test),
and every test asserts how many variants it ran.

  family           when                                           reason, from the launchers
  ---------------  ---------------------------------------------  ------------------------------------------
  conv epilogue    variant >= 20 with out= / bias= / gate= /      conv_kernel.hpp launch_rows_variant: the
                   acc_mask=                                      row-image kernel has the plain, statistics
                                                                  and BN-backward-sums epilogues only
  conv_wgrad       Cout % tile rows or Cin % tile columns         conv_wgrad.hip conv_wgrad_plan: "tile/channel
                   (0 128x128, 1 128x64, 2 64x128, 3 64x64,       mismatch"
                   4 256x128, 5 128x256, 7 256x256)
  conv_wgrad       variant 6 unless ks 3 and stride 1             conv_wgrad_plan: "rows variant needs 3x3/s1"
  gemm             variant 3 with N % 256                         conv_gemm.hip launch_gemm: "variant 3: N % 256"
  gemm_nt          bn 1128 / 1256 with K % 64                     gemm.hip launch_gemm_nt: "4-wave tiles need
                                                                  K % 64 == 0"

Left out by construction (nothing is launched, so nothing can be refused): gemm variant 0 with N % 256 (the
launcher falls through to the 128-wide tiles, which variants 1 and 2 cover); conv variants 7 / 8 on case C
(Cout = 64); conv_wgrad_rect row-image variants on stride 2 other than 8, 11, 12, 13 (variant 6 is stride-1
only) and wherever conv_wgrad_rows_rect_supported says no."""
import pytest
import torch

import exact_cases as X
from kungfu_amd.utils.numerics import assert_bits_equal

pytestmark = pytest.mark.gpu

_ROWS_EPI = ("out", "bias", "gate", "acc_mask", "acc_mask+bn_mask")
_WGRAD_TILE = {0: (128, 128), 1: (128, 64), 2: (64, 128), 3: (64, 64), 4: (256, 128), 5: (128, 256), 7: (256, 256)}

# (family, when(**kw), substring of the launcher's message)
REJECTIONS = [
    ("conv_epi", lambda variant, epi, **_: variant >= 20 and epi in _ROWS_EPI, "row-image variant unsupported"),
    ("conv_wgrad", lambda variant, Cin, Cout, **_: variant in _WGRAD_TILE and (
        Cout % _WGRAD_TILE[variant][0] != 0 or Cin % _WGRAD_TILE[variant][1] != 0), "tile/channel mismatch"),
    ("conv_wgrad", lambda variant, ks, stride, **_: variant == 6 and (ks != 3 or stride != 1),
     "rows variant needs 3x3/s1"),
    ("gemm", lambda variant, N, **_: variant == 3 and N % 256 != 0, "variant 3: N % 256"),
    ("gemm_nt", lambda bn, K, **_: bn > 1000 and K % 64 != 0, "4-wave tiles need K % 64"),
]


class Rejected:
    """What _call returns for a combination the launcher refused as REJECTIONS says."""


def _call(family, fn, **kw):
    """fn(), or Rejected when the launcher refuses the combination exactly as REJECTIONS lists it."""
    rule = next((r for r in REJECTIONS if r[0] == family and r[1](**kw)), None)
    try:
        out = fn()
    except (ValueError, RuntimeError) as e:
        assert rule is not None, "%s %r: rejection not in the REJECTIONS table: %s" % (family, kw, e)
        assert rule[2] in str(e), "%s %r: rejected with %r, the table says %r" % (family, kw, str(e), rule[2])
        return Rejected
    assert rule is None, "%s %r: listed in REJECTIONS (%s) but the launcher ran it" % (family, kw, rule[2])
    return out


@pytest.fixture(scope="module")
def H():
    from kungfu_amd._lib import hip

    return hip()


def _dev(t):
    """A CPU integer tensor as the kernels take it: bf16 on the GPU, channels_last when 4-D."""
    t = t.cuda().bfloat16()
    return t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t.contiguous()


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _stats(H, C):
    return torch.zeros(H.conv_stat_slots * 2 * C, dtype=torch.float64, device="cuda")


def _check_sums(st, C, s1, s2, what, times=1):
    """The slot-summed f64 statistics equal the f64 reference sums exactly (s2 None: the gate's one sum)."""
    sums = st.view(-1, 2, C).sum(0)
    assert_bits_equal(sums[0], s1 * times, what + " sum 1")
    if s2 is not None:
        assert_bits_equal(sums[1], s2 * times, what + " sum 2")
    else:
        assert not sums[1].any(), what + ": the second sum is not used"


def _pad2(ks):
    return (ks - 1) // 2


# ---- forward conv ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,ks,stride", X.FWD)
def test_conv_forward(H, name, ks, stride):
    N, Hh, W, Ci, Co = X.CONV[name]
    c = X.conv_case(N, Hh, W, Ci, Co, ks, ks, stride, _pad2(ks), _pad2(ks))
    x, w = _dev(c["x"]), _dev(c["w"])
    variants = X.C_VARIANTS if name == "C" else X.AB_VARIANTS
    ran = 0
    for v in variants:
        y = H.conv(x, w, stride, None, None, v)
        assert y.is_contiguous(memory_format=torch.channels_last)
        assert_bits_equal(y, c["ref"], "conv %s ks%d s%d variant %d [n, co, oh, ow]" % (name, ks, stride, v))
        ran += 1
    assert ran == (2 if name == "C" else 6)


@pytest.mark.parametrize("name,ks", X.V11)
def test_conv_forward_variant_11(H, name, ks):
    """The 256x32 tile: the default only for Cout <= 32 (reached through conv_rect, test_conv_rect), but
    conv(..., variant=11) runs it on any Cout as several 32-column tiles."""
    N, Hh, W, Ci, Co = X.CONV[name]
    c = X.conv_case(N, Hh, W, Ci, Co, ks, ks, 1, _pad2(ks), _pad2(ks))
    y = H.conv(_dev(c["x"]), _dev(c["w"]), 1, None, None, 11)
    assert_bits_equal(y, c["ref"], "conv %s ks%d variant 11" % (name, ks))


@pytest.mark.parametrize("name,ks,hi", X.FWD_TIES)
def test_conv_forward_rounds_ties_to_even(H, name, ks, hi):
    N, Hh, W, Ci, Co = X.CONV[name]
    c = X.conv_case(N, Hh, W, Ci, Co, ks, ks, 1, _pad2(ks), _pad2(ks), "ties", hi)
    x, w = _dev(c["x"]), _dev(c["w"])
    ran = 0
    for v in X.TIES_VARIANTS:
        assert_bits_equal(H.conv(x, w, 1, None, None, v), c["ref"], "conv ties ks%d variant %d" % (ks, v), ties=True)
        ran += 1
    assert ran == 3


@pytest.mark.parametrize("variant,N,Hh,W,Ci,Co", X.ROWS)
def test_conv_rows_forward_and_stats(H, variant, N, Hh, W, Ci, Co):
    c = X.stat_sums(X.conv_case(N, Hh, W, Ci, Co, 3, 3, 1, 1, 1), N * Hh * W)
    x, w = _dev(c["x"]), _dev(c["w"])
    what = "conv rows variant %d" % variant
    assert_bits_equal(H.conv(x, w, 1, None, None, variant), c["ref"], what)
    st = _stats(H, Co)
    assert_bits_equal(H.conv(x, w, 1, st, None, variant), c["ref"], what + " + stats")
    _check_sums(st, Co, c["s1"], c["s2"], what)


# ---- the epilogues of conv ------------------------------------------------------------------------------

@pytest.mark.parametrize("ks,variant,shape", X.EPI)
def test_conv_epilogues(H, ks, variant, shape):
    N, Hh, W, Ci, Co = shape
    c = X.epilogue_case(N, Hh, W, Ci, Co, ks)
    x, w = _dev(c["x"]), _dev(c["w"])
    old, bx, relu_out = _dev(c["old"]), _dev(c["bx"]), _dev(c["relu_out"])
    amask, bmask, fcoef = c["amask"].cuda(), c["bmask"].cuda(), c["fcoef"].cuda()
    what = "conv ks%d variant %d " % (ks, variant)
    ran, rejected = [], []

    def run(epi, fn):
        out = _call("conv_epi", fn, variant=variant, epi=epi)
        (rejected if out is Rejected else ran).append(epi)
        return out

    # forward statistics: exact sums; slots are only ever added to (a second call doubles them)
    st = _stats(H, Co)
    y = run("stats", lambda: H.conv(x, w, 1, st, None, variant))
    assert_bits_equal(y, c["ref"], what + "stats")
    _check_sums(st, Co, c["s1"], c["s2"], what + "stats")
    H.conv(x, w, 1, st, None, variant)
    _check_sums(st, Co, c["s1"], c["s2"], what + "stats, second call", times=2)
    # accumulate
    o = old.clone()
    if run("out", lambda: H.conv(x, w, 1, None, o, variant)) is not Rejected:
        assert_bits_equal(o, c["acc"], what + "out=")
    # relu(conv + bias)
    y = run("bias", lambda: H.conv(x, w, 1, None, None, variant, bias=_dev(c["bias"])))
    if y is not Rejected:
        assert_bits_equal(y, c["bias_relu"], what + "bias=")
    # gate by a ReLU output, one sum
    st = _stats(H, Co)
    y = run("gate", lambda: H.conv(x, w, 1, st, None, variant, bn_x=relu_out, gate=True))
    if y is not Rejected:
        assert_bits_equal(y, c["gated"], what + "gate")
        _check_sums(st, Co, c["gated_s1"], None, what + "gate")
    # out = old * acc_mask + conv, without and with the BN-backward sums from bn_mask
    o = old.clone()
    if run("acc_mask", lambda: H.conv(x, w, 1, None, o, variant, acc_mask=amask)) is not Rejected:
        assert_bits_equal(o, c["acc_mask"], what + "acc_mask")
    o, st = old.clone(), _stats(H, Co)
    if run("acc_mask+bn_mask", lambda: H.conv(x, w, 1, st, o, variant, bn_x=bx, bn_mask=bmask, acc_mask=amask)) \
            is not Rejected:
        assert_bits_equal(o, c["acc_mask"], what + "acc_mask + bn_mask")
        _check_sums(st, Co, c["am_s1"], c["am_s2"], what + "acc_mask + bn_mask")
    # BN-backward sums from the 1-bit mask and from the forward coefficients
    st = _stats(H, Co)
    y = run("bn_mask", lambda: H.conv(x, w, 1, st, None, variant, bn_x=bx, bn_mask=bmask))
    assert_bits_equal(y, c["ref"], what + "bn_mask")
    _check_sums(st, Co, c["mk_s1"], c["mk_s2"], what + "bn_mask")
    st = _stats(H, Co)
    y = run("bn_fcoef", lambda: H.conv(x, w, 1, st, None, variant, bn_x=bx, bn_fcoef=fcoef))
    assert_bits_equal(y, c["ref"], what + "bn_fcoef")
    _check_sums(st, Co, c["co_s1"], c["co_s2"], what + "bn_fcoef")
    assert (len(ran), len(rejected)) == ((3, 5) if variant >= 20 else (8, 0)), (ran, rejected)


# ---- data gradients -------------------------------------------------------------------------------------

@pytest.mark.parametrize("Co,Ci", X.S2_EVEN_PAIRS)
def test_conv_dgrad_s2_even_input(H, Co, Ci):
    """ks 3: four parity phases (1, 2, 2 and 4 taps) write every dx pixel once, on every phase tile, and with
    the BN-backward sums; ks 1: the even pixels, completed by the acc_even stride-1 data gradient."""
    N, OH, OW = X.S2_GRID
    c = X.dgrad_case(N, OH, OW, Co, Ci, 3, 2, 1, 2 * OH, 2 * OW)
    dy, wt = _dev(c["dy"]), H.conv_flip_weight(_dev(c["w"]))
    ran = 0
    for v in (-1, 0, 1, 2, 5):
        dx = H.conv_dgrad_s2(dy, wt, 3, variant=v)
        assert_bits_equal(dx, c["ref"], "conv_dgrad_s2 3x3 %d->%d tile %d [n, ci, h, w]" % (Co, Ci, v))
        ran += 1
    assert ran == 5
    st = _stats(H, Ci)
    dx = H.conv_dgrad_s2(dy, wt, 3, st, _dev(c["bx"]), c["fcoef"].cuda())
    assert_bits_equal(dx, c["ref"], "conv_dgrad_s2 3x3 + BN sums")
    _check_sums(st, Ci, c["co_s1"], c["co_s2"], "conv_dgrad_s2 3x3 BN sums")
    # the downsample pair: the other pixels of dx hold a sentinel until the acc_even conv stores them
    p = X.dgrad_pair_case(N, OH, OW, Co, Ci)
    dx = H.conv_dgrad_s2(_dev(p["dy2"]), H.conv_flip_weight(_dev(p["w2"])), 1)
    assert_bits_equal(dx[:, :, 0::2, 0::2], p["even"][:, :, 0::2, 0::2].contiguous(), "conv_dgrad_s2 1x1 even pixels")
    odd = torch.ones(2 * OH, 2 * OW, dtype=torch.bool, device="cuda")
    odd[0::2, 0::2] = False
    dx.permute(0, 2, 3, 1)[:, odd] = 99.0  # left undefined by the 1x1 phase: must be overwritten, not added to
    out = H.conv(_dev(p["dy1"]), H.conv_flip_weight(_dev(p["w1"])), 1, None, dx, acc_even=True)
    assert out.data_ptr() == dx.data_ptr()
    assert_bits_equal(dx, p["ref"], "conv_dgrad_s2 1x1 + acc_even conv [n, ci, h, w]")


@pytest.mark.parametrize("Co,Ci", X.S2_ANY_PAIRS)
@pytest.mark.parametrize("dh,dw,pad", X.S2_ANY)
def test_conv_dgrad_s2_any_size(H, dh, dw, pad, Co, Ci):
    N, OH, OW = X.S2_GRID
    c = X.dgrad_case(N, OH, OW, Co, Ci, 3, 2, pad, dh, dw)
    dy, wt = _dev(c["dy"]), H.conv_flip_weight(_dev(c["w"]))
    what = "conv_dgrad_s2 %dx%d pad %d %d->%d" % (dh, dw, pad, Co, Ci)
    assert_bits_equal(H.conv_dgrad_s2(dy, wt, 3, dh=dh, dw=dw, pad=pad), c["ref"], what)
    st = _stats(H, Ci)
    dx = H.conv_dgrad_s2(dy, wt, 3, st, _dev(c["bx"]), c["fcoef"].cuda(), None, -1, dh, dw, pad)
    assert_bits_equal(dx, c["ref"], what + " + BN sums")
    _check_sums(st, Ci, c["co_s1"], c["co_s2"], what + " BN sums")


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("ks", [1, 3])
def test_conv_dgrad_s1(H, name, ks):
    """conv_flip_weight, then conv, against conv2d_input."""
    N, Hh, W, Ci, Co = X.CONV[name]
    c = X.dgrad_case(N, Hh, W, Co, Ci, ks, 1, _pad2(ks), Hh, W)
    dy, wt = _dev(c["dy"]), H.conv_flip_weight(_dev(c["w"]))
    ran = 0
    for v in (-1, 0, 2):
        assert_bits_equal(H.conv(dy, wt, 1, None, None, v), c["ref"], "dgrad s1 %s ks%d variant %d" % (name, ks, v))
        ran += 1
    assert ran == 3


# ---- rectangular windows --------------------------------------------------------------------------------

@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("Co", X.RECT_COUT)
@pytest.mark.parametrize("kh,kw,ph,pw", X.RECT_WINDOWS)
def test_conv_rect(H, kh, kw, ph, pw, Co, stride):
    """Cout 192: 256x64 tiles; 128: 256x128; 32: the 256x32 tile (conv variant 11 as the default for Cout <= 32)."""
    N, Hh, W = X.RECT_IMAGE
    assert H.conv_rect_supported(X.RECT_CIN, Co, kh, kw, stride)
    OH, OW = (Hh + 2 * ph - kh) // stride + 1, (W + 2 * pw - kw) // stride + 1
    c = X.stat_sums(X.conv_case(N, Hh, W, X.RECT_CIN, Co, kh, kw, stride, ph, pw), N * OH * OW)
    x, w = _dev(c["x"]), _dev(c["w"])
    what = "conv_rect %dx%d s%d ->%d" % (kh, kw, stride, Co)
    assert_bits_equal(H.conv_rect(x, w, stride, ph, pw), c["ref"], what)
    st = _stats(H, Co)
    assert_bits_equal(H.conv_rect(x, w, stride, ph, pw, st), c["ref"], what + " + stats")
    _check_sums(st, Co, c["s1"], c["s2"], what)


# ---- weight gradients -----------------------------------------------------------------------------------

def _wgrad_variants(H, shape, ks, stride, fn):
    """fn(variant) for every variant below conv_wgrad_variants(); returns how many the planner accepted."""
    N, Ci, Hh, W, Co = shape
    ran = 0
    for v in range(H.conv_wgrad_variants()):
        if _call("conv_wgrad", lambda: H.conv_wgrad_plan(N, Hh, W, Ci, Co, ks, stride, v, -1), variant=v, Cin=Ci,
                 Cout=Co, ks=ks, stride=stride) is Rejected:
            continue
        fn(v)
        ran += 1
    return ran


_WGRAD_TILES_RAN = {(64, 256): 2, (192, 64): 1, (256, 256): 7}  # (Cin, Cout) -> tap-tiled variants accepted


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("ks", [1, 3])
@pytest.mark.parametrize("shape", X.WGRAD)
def test_conv_wgrad(H, shape, ks, stride):
    N, Ci, Hh, W, Co = shape
    c = X.wgrad_case(N, Ci, Hh, W, Co, ks, ks, stride, _pad2(ks), _pad2(ks))
    x, dy = _dev(c["x"]), _dev(c["dy"])
    base32 = _cl(c["base"].cuda())

    def run(v):
        for sp in (1, 3, -1):
            what = "conv_wgrad ks%d s%d %d->%d variant %d splits %d [co, ci, kh, kw] " % (ks, stride, Ci, Co, v, sp)
            assert_bits_equal(H.conv_wgrad(dy, x, ks, stride, variant=v, splits=sp), c["ref"], what + "bf16")
            o = torch.full_like(base32, 7.0)
            H.conv_wgrad(dy, x, ks, stride, out=o, variant=v, splits=sp)
            assert_bits_equal(o, c["ref"], what + "f32 out=")
            for atomics in (True, False):
                o = base32.clone()
                H.conv_wgrad(dy, x, ks, stride, out=o, accumulate=True, variant=v, splits=sp, atomics=atomics)
                assert_bits_equal(o, c["acc"], what + "f32 accumulate, atomics %s" % atomics)
                o = base32.bfloat16()
                H.conv_wgrad(dy, x, ks, stride, out=o, accumulate=True, variant=v, splits=sp, atomics=atomics)
                assert_bits_equal(o, c["acc"], what + "bf16 accumulate, atomics %s" % atomics)

    ran = _wgrad_variants(H, shape, ks, stride, run)
    run(-1)
    assert ran == _WGRAD_TILES_RAN[(Ci, Co)] + (1 if ks == 3 and stride == 1 else 0)


def test_conv_wgrad_rounds_ties_to_even(H):
    shape, ks, stride, hi = X.WGRAD_TIES
    N, Ci, Hh, W, Co = shape
    c = X.wgrad_case(N, Ci, Hh, W, Co, ks, ks, stride, 0, 0, "ties", hi)
    x, dy = _dev(c["x"]), _dev(c["dy"])

    def run(v):
        for sp in (1, 3, -1):
            assert_bits_equal(H.conv_wgrad(dy, x, ks, stride, variant=v, splits=sp), c["ref"],
                              "conv_wgrad ties variant %d splits %d" % (v, sp), ties=True)

    assert _wgrad_variants(H, shape, ks, stride, run) == 2
    run(-1)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("kh,kw,ph,pw", X.RECT_WINDOWS)
def test_conv_wgrad_rect(H, kh, kw, ph, pw, stride):
    """Channel counts that are multiples of 8 but not of 64, on the tap-tiled kernel and every row-image variant
    that covers the window."""
    N, Hh, W = X.WGRAD_RECT_IMAGE
    Ci, Co = X.WGRAD_RECT_CH
    assert H.conv_wgrad_rect_supported(Ci, Co, kh, kw, stride)
    c = X.wgrad_case(N, Ci, Hh, W, Co, kh, kw, stride, ph, pw)
    x, dy = _dev(c["x"]), _dev(c["dy"])
    variants = [-1]
    if H.conv_wgrad_rows_rect_supported(N, Hh, W, Ci, Co, kh, kw, ph, pw, stride):
        variants += [6, 8, 9, 10, 11, 12, 13] if stride == 1 else [8, 11, 12, 13]
    for v in variants:
        dw = H.conv_wgrad_rect(dy, x, kh, kw, stride, ph, pw, v)
        assert_bits_equal(dw, c["ref"], "conv_wgrad_rect %dx%d s%d variant %d [co, ci, kh, kw]" % (kh, kw, stride, v))
    # every window of the table is small enough for the row-image kernel on this image
    assert len(variants) == (8 if stride == 1 else 5)


# ---- GEMMs ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,K,N", X.GEMM)
def test_gemm(H, M, K, N):
    c = X.gemm_case(M, K, N)
    a, b, bias, old = _dev(c["a"]), _dev(c["b"]), _dev(c["bias"]), _dev(c["old"])
    variants = [-1, 1, 2, 3] + ([0] if N % 256 == 0 else [])
    ran = 0
    for v in variants:
        what = "gemm %dx%dx%d variant %d [m, n] " % (M, K, N, v)
        y = _call("gemm", lambda: H.gemm(a, b, variant=v)[0], variant=v, N=N)
        if y is Rejected:
            continue
        assert_bits_equal(y, c["ref"], what + "plain")
        assert_bits_equal(H.gemm(a, b, bias, variant=v)[0], c["with_bias"], what + "bias")
        o = old.clone()
        assert H.gemm(a, b, out=o, variant=v)[0].data_ptr() == o.data_ptr()
        assert_bits_equal(o, c["acc"], what + "out=")
        ran += 1
    assert ran == (5 if N % 256 == 0 else 3)


@pytest.mark.parametrize("K", X.GEMM_NT_K)
def test_gemm_nt(H, K):
    M, N = X.GEMM_NT_MN
    assert H.gemm_nt_supported(M, N, K) and (K > 32 or not H.gemm_nt_supported(M, N, K - 8))
    c = X.gemm_case(M, K, N)
    a, b, bias, old = _dev(c["a"]), _dev(c["b"]), _dev(c["bias"]), _dev(c["old"])
    ran = 0
    for bn in X.GEMM_NT_BN:
        what = "gemm_nt K %d bn %d [m, n] " % (K, bn)
        y = _call("gemm_nt", lambda: H.gemm_nt(a, b, bn=bn), bn=bn, K=K)
        if y is Rejected:
            continue
        assert_bits_equal(y, c["ref"], what + "plain")
        assert_bits_equal(H.gemm_nt(a, b, bias, bn=bn), c["with_bias"], what + "bias")
        o = old.clone()
        H.gemm_nt(a, b, out=o, accumulate=True, bn=bn)
        assert_bits_equal(o, c["acc"], what + "accumulate")
        o = old.clone()
        H.gemm_nt(a, b, bias, out=o, accumulate=True, bn=bn)
        assert_bits_equal(o, c["acc_bias"], what + "bias + accumulate")
        ran += 1
    assert ran == (6 if K % 64 == 0 else 4)


def test_gemm_nt_rounds_ties_to_even(H):
    (M, N), (K, hi) = X.GEMM_NT_MN, X.GEMM_NT_TIES
    c = X.gemm_case(M, K, N, "ties", hi)
    a, b = _dev(c["a"]), _dev(c["b"])
    for bn in X.GEMM_NT_BN:
        assert_bits_equal(H.gemm_nt(a, b, bn=bn), c["ref"], "gemm_nt ties bn %d" % bn, ties=True)


@pytest.mark.parametrize("M,K,N", X.GEMM_NT_LD)
def test_gemm_nt_ld_ragged(H, M, K, N):
    c = X.gemm_case(M, K, N)
    a, b, bias = _dev(c["a"]), _dev(c["b"]), _dev(c["bias"])
    ld = (N + 7) // 8 * 8 + 16
    for bn in (128, 192, 256):
        what = "gemm_nt_ld %dx%dx%d bn %d [m, n] " % (M, K, N, bn)
        y = H.gemm_nt_ld(a, b, bias, ld, bn)
        assert y.shape == (M, ld)
        assert_bits_equal(y[:, :N], c["with_bias"], what + "bias, padded rows")  # columns >= N: unspecified
        y = H.gemm_nt_ld(a, b, None, 0, bn)
        assert y.shape == (M, (N + 7) // 8 * 8)
        assert_bits_equal(y[:, :N], c["ref"], what + "plain")


# ---- stems ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,Hh,W", X.STEM_IMAGES)
def test_stem_forward_and_wgrad(H, N, Hh, W):
    OH, OW = (Hh - 1) // 2 + 1, (W - 1) // 2 + 1
    c = X.stat_sums(X.conv_case(N, Hh, W, 3, 64, 7, 7, 2, 3, 3), N * OH * OW)
    wp = H.stem_pack_weight(_dev(c["w"]))
    for img in (_dev(c["x"]), _cl(c["x"].cuda())):  # bf16 and f32 image
        st = _stats(H, 64)
        y = H.stem_forward(H.stem_pad4(img), wp, st)
        assert_bits_equal(y, c["ref"], "stem_forward %dx%d from %s [n, co, oh, ow]" % (Hh, W, img.dtype))
        _check_sums(st, 64, c["s1"], c["s2"], "stem_forward %dx%d" % (Hh, W))
    g = X.wgrad_case(N, 3, Hh, W, 64, 7, 7, 2, 3, 3, "dense_x")
    x4, dy = H.stem_pad4(_dev(g["x"])), _dev(g["dy"])
    for sp in (-1, 1):
        dw = H.stem_wgrad(dy, x4, sp)
        assert_bits_equal(dw, g["ref"], "stem_wgrad %dx%d splits %d [co, c, kh, kw]" % (Hh, W, sp))


@pytest.mark.parametrize("n,h,w,k,s,p", X.STEM3)
def test_stem3_forward_and_wgrad(H, n, h, w, k, s, p):
    OH, OW = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    c = X.stat_sums(X.conv_case(n, h, w, 3, 32, k, k, s, p, p), n * OH * OW)
    wp = H.stem3_pack_weight(_dev(c["w"]))
    for img in (_dev(c["x"]), _cl(c["x"].cuda())):  # bf16 and f32 image
        st = _stats(H, 32)
        y = H.stem3_forward(img, wp, k, k, s, p, p, st)
        assert_bits_equal(y, c["ref"], "stem3_forward %dx%d k%d from %s" % (h, w, k, img.dtype))
        _check_sums(st, 32, c["s1"], c["s2"], "stem3_forward %dx%d" % (h, w))
    g = X.wgrad_case(n, 3, h, w, 32, k, k, s, p, p, "dense_x")
    dy = _dev(g["dy"])
    for img in (_dev(g["x"]), _cl(g["x"].cuda())):
        what = "stem3_wgrad %dx%d k%d from %s " % (h, w, k, img.dtype)
        assert_bits_equal(H.stem3_wgrad(dy, img, k, k, s, p, p, out_f32=True), g["ref"], what + "f32")
        assert_bits_equal(H.stem3_wgrad(dy, img, k, k, s, p, p), g["ref"], what + "bf16")


# ---- guard rows: a tail tile must not store past M ------------------------------------------------------

_GUARD = 512  # rows past M: more than the tallest tile


def _guarded(rows_shape, lead, fill, dtype=torch.bfloat16, channels_last=False):
    """A buffer of lead + guard leading entries: its first ``lead`` entries (the view handed to the binding)
    and a copy of the sentinel rows behind them."""
    per = 1
    for d in rows_shape[2:]:
        per *= d
    extra = (_GUARD + per - 1) // per
    big = torch.full((lead + extra,) + tuple(rows_shape[1:]), -776.0, dtype=dtype, device="cuda")
    if channels_last:
        big = _cl(big)
    big[:lead] = fill
    return big, big[:lead], big[lead:].clone()


def test_guard_rows_conv(H):
    for ks in (1, 3):
        N, Hh, W, Ci, Co = X.CONV["A"]
        c = X.epilogue_case(N, Hh, W, Ci, Co, ks)
        x, w = _dev(c["x"]), _dev(c["w"])
        for v in X.AB_VARIANTS:
            big, out, guard = _guarded(c["ref"].shape, N, _dev(c["old"]), channels_last=True)
            assert out.is_contiguous(memory_format=torch.channels_last)
            H.conv(x, w, 1, None, out, v)
            assert_bits_equal(out, c["acc"], "guarded conv ks%d variant %d" % (ks, v))
            assert torch.equal(big[N:], guard), "conv ks%d variant %d stored past M" % (ks, v)


def test_guard_rows_gemm(H):
    for M, K, N in X.GEMM:
        c = X.gemm_case(M, K, N)
        a, b = _dev(c["a"]), _dev(c["b"])
        for v in [-1, 1, 2] + ([0, 3] if N % 256 == 0 else []):
            big, out, guard = _guarded((M, N), M, _dev(c["old"]))
            H.gemm(a, b, out=out, variant=v)
            assert_bits_equal(out, c["acc"], "guarded gemm %dx%dx%d variant %d" % (M, K, N, v))
            assert torch.equal(big[M:], guard), "gemm %dx%dx%d variant %d stored past M" % (M, K, N, v)


def test_guard_rows_gemm_nt(H):
    M, N = X.GEMM_NT_MN
    c = X.gemm_case(M, 192, N)
    a, b = _dev(c["a"]), _dev(c["b"])
    for bn in X.GEMM_NT_BN:
        for accumulate in (False, True):
            big, out, guard = _guarded((M, N), M, _dev(c["old"]))
            H.gemm_nt(a, b, out=out, accumulate=accumulate, bn=bn)
            assert_bits_equal(out, c["acc"] if accumulate else c["ref"], "guarded gemm_nt bn %d" % bn)
            assert torch.equal(big[M:], guard), "gemm_nt bn %d stored past M" % bn


def test_guard_rows_conv_wgrad(H):
    """dw's rows are the output channels: the sentinel rows follow channel Cout - 1."""
    for shape in X.WGRAD:
        N, Ci, Hh, W, Co = shape
        for ks in (1, 3):
            c = X.wgrad_case(N, Ci, Hh, W, Co, ks, ks, 1, _pad2(ks), _pad2(ks))
            x, dy = _dev(c["x"]), _dev(c["dy"])

            def run(v):
                for dtype in (torch.bfloat16, torch.float32):
                    big, out, guard = _guarded(c["ref"].shape, Co, c["base"].cuda().to(dtype), dtype, True)
                    assert out.is_contiguous(memory_format=torch.channels_last)
                    H.conv_wgrad(dy, x, ks, 1, out=out, accumulate=True, variant=v)
                    assert_bits_equal(out, c["acc"], "guarded conv_wgrad ks%d variant %d %s" % (ks, v, dtype))
                    assert torch.equal(big[Co:], guard), "conv_wgrad ks%d variant %d stored past Cout" % (ks, v)

            _wgrad_variants(H, shape, ks, 1, run)
            run(-1)
