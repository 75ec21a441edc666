"""Bit-exact tests of the conv epilogue's f32 -> bf16 rounding (cvt_pk_bf16, common.hpp) and of the conv
kernels' pixel addressing (the decode-free 1x1 path and the reciprocal-division decodes, conv_kernel.hpp)
on the recipes of tests/rounding_cases.py: 0/1 weights with two ones per output channel, so every
accumulator is an exactly known f32 sum of two bf16 inputs and the reference is that value rounded by torch
on the CPU.  tests/test_rounding_cases.py checks the recipe itself without a GPU.

Shapes: N = 2 at 8 x 8 and 9 x 9 (a ragged last tile, tiles spanning two images), N = 3 at 5 x 5 and 7 x 11
(tiles crossing image and row boundaries at every offset), Cin 64, Cout 64 / 128 / 256, every tile variant
the shape admits (the row-image variants 24 and 25 for 3x3).  Persistent-branch cases, the smallest M by the rule
in launch_epi / launch_rows_epi (statistics epilogue and mtiles > 2 * per_n, per_n = 256 * OCC / ntiles):
  * conv_kernel, 256 x 256 tiles (variant 7: 128 KB of LDS, OCC = 1), Cout = 1024: ntiles = 4, per_n = 64, so
    mtiles > 128, M > 32768: M = 32769 = 1 * 99 * 331 pixels, 129 m-tiles (1x1: the decode-free path; 3x3: the
    tap-wise decode);
  * conv_rows_kernel (variants 24 and 25: 80 KB, OCC = 2), Cout = 64: ntiles = 1, per_n = 512, so mtiles > 1024,
    M > 262144: M = 262145 = 65 * 109 * 37 pixels, 1025 m-tiles."""
import functools

import pytest
import torch

import rounding_cases as R

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

CL = torch.channels_last
ROUNDING_SHAPES = [(2, 8, 8), (2, 9, 9)]
ADDRESS_SHAPES = ROUNDING_SHAPES + [(3, 5, 5), (3, 7, 11)]
COUTS = [64, 128, 256]


@pytest.fixture(scope="module")
def H():
    from kungfu_amd._lib import hip

    return hip()


def _dev(t):
    return t.cuda().contiguous(memory_format=CL)


def variants(cout, ks, rows_ok=True):
    """The tile variants a [.., 64 -> cout] conv admits (launch_ks / launch_rows in conv_k3.hip)."""
    v = [-1, 2, 11]
    if cout % 128 == 0:
        v += [0, 1]
    if cout % 256 == 0:
        v += [7, 8]
    if ks == 3 and cout % 64 == 0 and rows_ok:
        v += [24, 25]
    return v


@functools.lru_cache(maxsize=None)
def rounding_x(shape, finite=False):
    return R.rounding_input(*shape, finite=finite)


@functools.lru_cache(maxsize=None)
def reference(kind, shape, cout, ks, stride=1, centre=True):
    """(x on the CPU, the exact f32 accumulators, their bf16 rounding by torch on the CPU)."""
    x = {"round": lambda: rounding_x(shape), "finite": lambda: rounding_x(shape, True),
         "pos": lambda: R.position_input(*shape), "nan": lambda: R.nan_input(*shape)}[kind]()
    v = R.conv_sum(x, cout, ks, stride, centre)
    return x, v, v.bfloat16()


def same_bits(got, want, what):
    """Bit equality; a NaN equals any NaN (inf - inf in an accumulate: the payload is the adder's choice)."""
    g, w = R.to_bits(got), R.to_bits(want)
    g = torch.where(torch.isnan(got.detach().cpu().float()), torch.full_like(g, 0x7fc0), g)
    w = torch.where(torch.isnan(want.float()), torch.full_like(w, 0x7fc0), w)
    if not torch.equal(g, w):
        bad = (g != w).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError("%s: %d of %d elements differ, first at [n, c, h, w] = %s: got 0x%04x, want 0x%04x" %
                             (what, bad.shape[0], g.numel(), i, g[i].item(), w[i].item()))


def stats_buf(H, K):
    return torch.zeros(H.conv_stat_slots * 2 * K, dtype=torch.float64, device="cuda")


def sums_of(st, K):
    return st.view(-1, 2, K).sum(0).cpu()


def check_sums(st, K, a, b, rows, what):
    """st's two f64 rows against the f64 sums of a and of a * b ([N, K, H, W] float64 on the CPU).  The kernels
    add f32 terms in f32 per thread (at most `rows` of them) before the f64 reduction, so each sum is within
    rows * 2^-24 * sum |term| of the exact one, plus one rounding per product."""
    got = sums_of(st, K)
    for i, t in enumerate((a, a * b)):
        t = t.permute(1, 0, 2, 3).reshape(K, -1)
        err = (got[i] - t.sum(1)).abs()
        bound = (rows + 1) * 2.0 ** -24 * t.abs().sum(1)
        assert (err <= bound).all(), "%s: sum %d off by %.3g, bound %.3g" % (what, i, err.max().item(),
                                                                          bound[err.argmax()].item())


# ---- rounding: plain and every fused epilogue, bit for bit


@pytest.mark.parametrize("shape", ROUNDING_SHAPES)
@pytest.mark.parametrize("cout", COUTS)
@pytest.mark.parametrize("ks", [1, 3])
def test_rounding_plain(H, shape, cout, ks):
    x, _, want = reference("round", shape, cout, ks)
    xd, wd = _dev(x), _dev(R.weights(cout, ks))
    for var in variants(cout, ks):
        same_bits(H.conv(xd, wd, 1, None, None, var), want, "variant %d" % var)


@pytest.mark.parametrize("shape", ROUNDING_SHAPES)
@pytest.mark.parametrize("ks", [1, 3])
def test_nan_inputs_stay_nan(H, shape, ks):
    """A NaN input reaches the outputs of its pixel (0 * NaN = NaN in every channel) as a NaN; every other
    element keeps its bits."""
    for centre in (True, False):
        x, v, want = reference("nan", shape, 128, ks, 1, centre)
        nan = torch.isnan(v)
        assert nan.any() and not nan.all()
        xd, wd = _dev(x), _dev(R.weights(128, ks, centre))
        for var in variants(128, ks):
            y = H.conv(xd, wd, 1, None, None, var).cpu()
            # the pixels a NaN input touches: every tap of the window multiplies it, by zero or one
            touched = torch.isnan(torch.nn.functional.conv2d(x.float(), torch.ones(1, R.CIN, ks, ks),
                                                             padding=(ks - 1) // 2)).expand_as(y)
            assert torch.isnan(y.float())[touched].all(), "variant %d: a NaN input came out as a number" % var
            assert not torch.isnan(y.float())[~touched].any()
            same_bits(torch.where(touched, torch.zeros_like(y), y), torch.where(touched, torch.zeros_like(y), want),
                      "variant %d, untouched pixels" % var)


@pytest.mark.parametrize("shape", ROUNDING_SHAPES)
@pytest.mark.parametrize("cout", COUTS)
@pytest.mark.parametrize("ks", [1, 3])
def test_rounding_stats(H, shape, cout, ks):
    """stats=: the outputs keep their bits, the sums are those of the ROUNDED outputs (finite inputs whose
    squares stay in f32 range)."""
    x, _, want = reference("finite", shape, cout, ks)
    xd, wd = _dev(x), _dev(R.weights(cout, ks))
    yd = want.double()
    for var in variants(cout, ks):
        st = stats_buf(H, cout)
        same_bits(H.conv(xd, wd, 1, st, None, var), want, "variant %d" % var)
        check_sums(st, cout, yd, yd, shape[0] * shape[1] * shape[2], "variant %d" % var)


def _old_for(r1, x):
    """An accumulate target for the rounded conv output r1: half an ulp of r1 on the even channels (the second
    rounding then sits on an exact tie, the even neighbour below or above by r1's last bit), recipe values of
    x on the odd ones."""
    b = R.to_bits(r1)
    expo = (b >> 7) & 0xff
    half = torch.where((expo > 8) & (expo < 255), (b & 0x8000) | ((expo - 8) << 7), torch.zeros_like(b))
    old = R.from_bits(half.numpy().astype("uint16"))
    reps = r1.shape[1] // x.shape[1]
    old[:, 1::2] = x.repeat(1, reps, 1, 1)[:, 1::2]
    return old


@pytest.mark.parametrize("shape", ROUNDING_SHAPES)
@pytest.mark.parametrize("cout", COUTS)
@pytest.mark.parametrize("ks", [1, 3])
def test_rounding_accumulate(H, shape, cout, ks):
    """out=: y = bf16(bf16(conv) + old), and with acc_mask old is first cleared where its bit is 0."""
    x, _, r1 = reference("round", shape, cout, ks)
    xd, wd = _dev(x), _dev(R.weights(cout, ks))
    old = _old_for(r1, x)
    want = (r1.float() + old.float()).bfloat16()
    assert (R.to_bits(want) != R.to_bits(r1)).any()
    torch.manual_seed(5)
    mask = torch.randint(0, 256, (old.numel() // 8,), dtype=torch.uint8)
    bits = ((mask.view(-1, 1) >> torch.arange(8)) & 1).bool().view(shape[0], shape[1], shape[2], cout).permute(0, 3, 1, 2)
    want_m = (r1.float() + torch.where(bits, old.float(), torch.zeros(()))).bfloat16()
    for var in variants(cout, ks, rows_ok=False):
        same_bits(H.conv(xd, wd, 1, None, _dev(old).clone(), var), want, "out=, variant %d" % var)
        same_bits(H.conv(xd, wd, 1, None, _dev(old).clone(), var, acc_mask=mask.cuda()), want_m,
                  "out= + acc_mask, variant %d" % var)


@pytest.mark.parametrize("shape", ROUNDING_SHAPES)
@pytest.mark.parametrize("cout", COUTS)
@pytest.mark.parametrize("ks", [1, 3])
def test_rounding_bn_backward(H, shape, cout, ks):
    """bn_x + bn_mask / bn_fcoef: the output keeps its bits (alone and accumulated through acc_mask), the sums
    are sum(dz) and sum(dz * x) of the rounded output, dz = y where the ReLU passed."""
    x, _, want = reference("finite", shape, cout, ks)
    xd, wd = _dev(x), _dev(R.weights(cout, ks))
    n = want.numel()
    torch.manual_seed(6)
    bx = (torch.randint(-8, 9, tuple(want.shape)).float() * 0.25).bfloat16()
    bmask = torch.randint(0, 256, (n // 8,), dtype=torch.uint8)
    nhwc = (shape[0], shape[1], shape[2], cout)
    on_bits = ((bmask.view(-1, 1) >> torch.arange(8)) & 1).bool().view(nhwc).permute(0, 3, 1, 2)
    fc = torch.cat([torch.randint(1, 5, (cout,)).float() * 0.5, torch.randint(-4, 5, (cout,)).float() * 0.25])
    on_coef = bx.float() * fc[:cout].view(1, -1, 1, 1) + fc[cout:].view(1, -1, 1, 1) > 0
    rows = shape[0] * shape[1] * shape[2]
    yd, bxd = want.double(), bx.double()
    for var in variants(cout, ks):
        for on, kw in ((on_bits, dict(bn_mask=bmask.cuda())), (on_coef, dict(bn_fcoef=fc.cuda()))):
            st = stats_buf(H, cout)
            same_bits(H.conv(xd, wd, 1, st, None, var, bn_x=_dev(bx), **kw), want, "variant %d %s" % (var, list(kw)))
            check_sums(st, cout, torch.where(on, yd, torch.zeros((), dtype=torch.float64)), bxd, rows,
                       "variant %d %s" % (var, list(kw)))
    # accumulate through the ReLU bits + BN-backward bits (the identity block's conv1 data gradient)
    old = _old_for(want, x)
    amask = torch.randint(0, 256, (n // 8,), dtype=torch.uint8)
    abits = ((amask.view(-1, 1) >> torch.arange(8)) & 1).bool().view(nhwc).permute(0, 3, 1, 2)
    want_a = (want.float() + torch.where(abits, old.float(), torch.zeros(()))).bfloat16()
    for var in variants(cout, ks, rows_ok=False):
        st = stats_buf(H, cout)
        same_bits(H.conv(xd, wd, 1, st, _dev(old).clone(), var, bn_x=_dev(bx), bn_mask=bmask.cuda(),
                         acc_mask=amask.cuda()), want_a, "acc_mask + bn_mask, variant %d" % var)
        check_sums(st, cout, torch.where(on_bits, want_a.double(), torch.zeros((), dtype=torch.float64)), bxd, rows,
                   "acc_mask + bn_mask, variant %d" % var)


@pytest.mark.parametrize("shape", ROUNDING_SHAPES)
@pytest.mark.parametrize("cout", COUTS)
@pytest.mark.parametrize("ks", [1, 3])
def test_rounding_bias_and_gate(H, shape, cout, ks):
    x, v, want = reference("finite", shape, cout, ks)
    xd, wd = _dev(x), _dev(R.weights(cout, ks))
    torch.manual_seed(7)
    # bias: relu(acc + bias) in f32, then ONE rounding (NaN-free inputs)
    bias = (torch.randint(-64, 65, (cout,)).float() * 2.0 ** -6).bfloat16()
    s = v + bias.float().view(1, -1, 1, 1)
    want_b = torch.where(s <= 0, torch.zeros(()), s).bfloat16()
    # gate: the rounded output where the ReLU output bx is positive, +0 elsewhere; stats[0] = its sum
    bx = (torch.randint(-2, 3, tuple(want.shape)).float()).bfloat16()
    keep = bx.float() > 0
    want_g = torch.where(keep, want, torch.zeros((), dtype=torch.bfloat16))
    rows = shape[0] * shape[1] * shape[2]
    for var in variants(cout, ks, rows_ok=False):
        same_bits(H.conv(xd, wd, 1, None, None, var, bias=bias.cuda()), want_b, "bias, variant %d" % var)
        st = stats_buf(H, cout)
        same_bits(H.conv(xd, wd, 1, st, None, var, bn_x=_dev(bx), gate=True), want_g, "gate, variant %d" % var)
        got = sums_of(st, cout)[0]
        t = want_g.double().permute(1, 0, 2, 3).reshape(cout, -1)
        assert ((got - t.sum(1)).abs() <= (rows + 1) * 2.0 ** -24 * t.abs().sum(1)).all(), "gate sums, variant %d" % var


@pytest.mark.parametrize("shape", ROUNDING_SHAPES)
@pytest.mark.parametrize("cout", COUTS)
@pytest.mark.parametrize("ks", [1, 3])
def test_rounding_one_ulp_from_a_tie(H, shape, cout, ks):
    """Sums one f32 ulp either side of an exact tie (low bits 0x8001 / 0x7fff), which need the bias epilogue's
    third term (rounding_cases.one_ulp_input): above the tie rounds up, below it rounds down."""
    x, bias = R.one_ulp_input(*shape), R.one_ulp_bias(cout)
    s = R.conv_sum(x, cout, ks) + bias.float().view(1, -1, 1, 1)
    low = s.contiguous().view(torch.int32) & 0xffff
    assert (low == 0x8001).sum() >= R.MIN_PER_CLASS and (low == 0x7fff).sum() >= R.MIN_PER_CLASS
    assert ((low == 0x8001) | (low == 0x7fff)).all()
    want = s.bfloat16()
    up = (R.to_bits(want).view_as(low) << 16) > s.contiguous().view(torch.int32)
    assert torch.equal(up, low == 0x8001)
    xd, wd = _dev(x), _dev(R.weights(cout, ks))
    for var in variants(cout, ks, rows_ok=False):
        same_bits(H.conv(xd, wd, 1, None, None, var, bias=bias.cuda()), want, "variant %d" % var)


@pytest.mark.parametrize("shape", ROUNDING_SHAPES)
@pytest.mark.parametrize("cin", [64, 128])
def test_rounding_dgrad_s2(H, shape, cin):
    """conv_dgrad_s2 for both kernel sizes on the rounding data (dy: 64 channels; dx: cin channels at twice the
    size), and the 1x1 + acc_even pair that completes a stride-2 1x1 data gradient."""
    dy, _, r = reference("round", shape, cin, 1)
    N, Hh, Ww = shape
    dyd = _dev(dy)
    for ks in (1, 3):
        wt = _dev(R.weights(cin, ks))  # [dx channels, dy channels, ks, ks]: the flipped layout, centre taps
        for var in (-1, 0, 1, 2, 5):
            dx = H.conv_dgrad_s2(dyd, wt, ks, variant=var).cpu()
            same_bits(dx[:, :, ::2, ::2], r, "ks %d variant %d, even pixels" % (ks, var))
            if ks == 3:  # every pixel written: the odd ones see no centre tap
                z = dx.clone()
                z[:, :, ::2, ::2] = 0
                assert (R.to_bits(z) == 0).all(), "ks 3 variant %d: odd pixels must be +0" % var
    # 1x1 pair: dx even pixels from conv_dgrad_s2, then a stride-1 1x1 data gradient accumulated with acc_even
    g2, _, r2 = reference("round", (N, 2 * Hh, 2 * Ww), cin, 1)
    wt = _dev(R.weights(cin, 1))
    want = r2.clone()
    want[:, :, ::2, ::2] = (r2[:, :, ::2, ::2].float() + r.float()).bfloat16()
    for var in variants(cin, 1):
        dx = H.conv_dgrad_s2(dyd, wt, 1)
        same_bits(H.conv(_dev(g2), wt, 1, None, dx, var, acc_even=True), want, "acc_even, variant %d" % var)


# ---- addressing: inputs that encode their own position


@pytest.mark.parametrize("shape", ADDRESS_SHAPES)
@pytest.mark.parametrize("cout", COUTS)
@pytest.mark.parametrize("ks", [1, 3])
def test_addressing(H, shape, cout, ks):
    x, v, want = reference("pos", shape, cout, ks, 1, False)
    assert torch.equal(want.float(), v)
    xd, wd = _dev(x), _dev(R.weights(cout, ks, False))
    yd = want.double()
    for var in variants(cout, ks, rows_ok=shape[2] >= 7):
        same_bits(H.conv(xd, wd, 1, None, None, var), want, "variant %d" % var)
        st = stats_buf(H, cout)
        same_bits(H.conv(xd, wd, 1, st, None, var), want, "stats, variant %d" % var)
        got = sums_of(st, cout)  # small integers: the f32 partial sums are exact
        assert torch.equal(got[0], yd.sum((0, 2, 3))) and torch.equal(got[1], (yd * yd).sum((0, 2, 3))), var


@pytest.mark.parametrize("shape", [(2, 8, 8), (3, 7, 11)])
def test_addressing_stride2_forward(H, shape):
    """A stride-2 1x1 (and 3x3) forward reads every other pixel: never the decode-free path."""
    for ks in (1, 3):
        x, v, want = reference("pos", shape, 128, ks, 2, False)
        xd, wd = _dev(x), _dev(R.weights(128, ks, False))
        for var in variants(128, ks, rows_ok=False):
            same_bits(H.conv(xd, wd, 2, None, None, var), want, "ks %d variant %d" % (ks, var))


@pytest.mark.parametrize("shape", ADDRESS_SHAPES)
def test_addressing_dgrad_s2(H, shape):
    """The scattering store decode of the stride-2 data-gradient phases against torch's transposed conv."""
    dy = R.position_input(*shape)
    for ks in (1, 3):
        wt = R.weights(128, ks, False)  # wt[ci, co, a, b] = w[co, ci, ks-1-a, ks-1-b]
        w_fwd = wt.float().flip(2, 3).permute(1, 0, 2, 3).contiguous()  # [dy channels, dx channels, kh, kw]
        want = torch.nn.functional.conv_transpose2d(dy.float(), w_fwd, stride=2, padding=(ks - 1) // 2,
                                                    output_padding=1)
        for var in (-1, 0, 1, 2, 5):
            dx = H.conv_dgrad_s2(_dev(dy), _dev(wt), ks, variant=var).cpu()
            if ks == 1:
                same_bits(dx[:, :, ::2, ::2], want[:, :, ::2, ::2].bfloat16(), "ks 1 variant %d" % var)
            else:
                same_bits(dx, want.bfloat16(), "ks 3 variant %d" % var)


def test_addressing_gemm(H):
    """The linear-layer binding runs the decode-free instances: rows are pixels of a 1 x 1 image."""
    x = R.position_input(300, 1, 1).reshape(300, R.CIN).contiguous()
    w = R.weights(128, 1).reshape(128, R.CIN).contiguous()
    want = (x.float() @ w.float().t()).bfloat16()
    for var in (-1, 1, 2):
        y = H.gemm(x.cuda(), w.cuda(), variant=var)[0]
        assert torch.equal(R.to_bits(y), R.to_bits(want)), var


# ---- the persistent branches (the M of each case: module docstring)


@pytest.mark.parametrize("ks", [1, 3])
def test_persistent_conv_kernel(H, ks):
    shape, cout = (1, 99, 331), 1024
    assert shape[0] * shape[1] * shape[2] == 32769 and (32769 + 255) // 256 == 2 * (256 // (cout // 256)) + 1
    x, v, want = reference("pos", shape, cout, ks, 1, False)
    st = stats_buf(H, cout)
    same_bits(H.conv(_dev(x), _dev(R.weights(cout, ks, False)), 1, st, None, 7), want, "ks %d" % ks)
    yd, got = want.double(), sums_of(st, cout)
    assert torch.equal(got[0], yd.sum((0, 2, 3))) and torch.equal(got[1], (yd * yd).sum((0, 2, 3)))


@pytest.mark.parametrize("var", [24, 25])
def test_persistent_conv_rows_kernel(H, var):
    shape, cout = (65, 109, 37), 64
    assert shape[0] * shape[1] * shape[2] == 262145 and (262145 + 255) // 256 == 2 * 512 + 1
    x, v, want = reference("pos", shape, cout, 3, 1, False)
    st = stats_buf(H, cout)
    same_bits(H.conv(_dev(x), _dev(R.weights(cout, 3, False)), 1, st, None, var), want, "rows")
    yd, got = want.double(), sums_of(st, cout)
    assert torch.equal(got[0], yd.sum((0, 2, 3))) and torch.equal(got[1], (yd * yd).sum((0, 2, 3)))
