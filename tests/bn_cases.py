"""Inputs, float64 references, assertions and a plain-torch emulation of the fused BatchNorm kernels
(csrc/kernels/bn.hip) for tests/test_gpu_bn_exact.py (the kernels) and tests/test_bn_cases.py (the
emulation and its mutants, on the CPU).

Nothing here imports the HIP extension.  Every function works on the device of its arguments, so the GPU
tests evaluate the f64 references on the GPU and the CPU tests run the very same assertions.

Data.  x, dy and the residual are small integers (kungfu_amd.utils.numerics.integer_data), so every
per-chunk f32 sum of x, x^2, dz and dz * x is an exact integer below 2^24 (asserted on the reference,
check_case) and the statistics must come out bit for bit: mean = float32(sum / rows), dbeta = sum dz.
The small shapes use integers in [-7, 8] (x) and [-3, 4] (dy, res); the two large shapes use the "dense"
values {-2, -1, 1, 2}.  In every case channel CONST_CH is constant (variance exactly 0, invstd =
1 / sqrt(eps)), channel NEAR_CH is constant except for the last element of the last row (variance
about 1 / rows: eps carries weight, and a dropped last row changes the statistics), and every 7th gamma
is negative.  gamma, beta, the running statistics and momentum (0.1) are general f32 values.

References are staged: each stage takes the kernel's own upstream f32 outputs (mean, invstd, coef,
dgamma, dbeta) as inputs, so no tolerance accumulates.  A bf16 output is checked with
kungfu_amd.utils.numerics.assert_rounds_from: delta = 2^-24 * k * (sum of the magnitudes of the terms),
k = the f32 roundings of the path counted on the uncontracted form of the kernel source:

  forward apply      K_FWD = 3      x * scale (1) + shift (1) [+ res (1)]
  forward, res_coef  K_FWD_RC = 5   shift + rshift (1), x * scale (1), + (1), res * rscale (1), + (1)
  backward apply     K_BWD = 16     a = gamma * invstd (1), 1 / rows (1), k2 = -a * dg * invstd / rows (3),
                                    k3 = -a * db / rows - k2 * mean (4), dx = k1 * dz + k2 * x + k3 (4): 13,
                                    taken as 16 (the coefficients' errors are counted once per use)
  backward, eval     K_BWD_EVAL = 3 a (1), a * dz (1), and one to spare

Observed shares of ambiguous elements (lo != hi in assert_rounds_from) with the committed seeds and salts
(SALT), on the emulation's coefficients.  The cap is 1 % everywhere; tests/test_bn_cases.py asserts it for every
recipe and prints the largest figures (test_ambiguous_shares_of_the_recipes):

  forward, every variant and shape          <= 1.2e-3   (simulation with randn data: 6.3e-4)
  backward dx, every variant and shape      <= 4.8e-3   (simulation with randn data: 1.7e-3)
  the two large shapes (ReLU variants)      0           (dense data: a few hundred distinct values)
  stem pool forward y / backward dx         0 / <= 3.2e-3
  single-row shapes, forward and backward   0           (48 and 64 elements: one would already pass 1 %)

With a single row every channel is constant: in training mode y = beta in exact arithmetic, as a difference
of terms 1 / sqrt(eps) = 316 times larger.  With gamma of order 1, delta is then of the order of the bf16
spacing of the result and most elements are ambiguous, so the single-row recipes scale gamma by
GAMMA_SINGLE_ROW = 2^-8, about sqrt(eps): scale and shift stay of order 1 and delta about 1e-6.  For the
same reason gamma, beta and the res_coef pair of the constant channel of every other recipe are fixed values
that keep its outputs well inside a bf16 interval (CONST_GAMMA, CONST_BETA)."""
import functools
import zlib

import torch

from kungfu_amd.utils.numerics import assert_bits_equal, assert_rounds_from, integer_data, ulp_of, unpack_mask

U = 2.0 ** -24
K_FWD, K_FWD_RC, K_BWD, K_BWD_EVAL = 3, 5, 16, 3
INVSTD_ULPS = 8  # rsqrtf (HIP documents 1 ulp) + a flip of float32(var) + the f32 add of eps, doubled
MOMENTUM, EPS = 0.1, 1e-5
CONST_CH, NEAR_CH = 1, 2
CONST_BETA, CONST_GAMMA = 0.7501, 0.625
GAMMA_SINGLE_ROW = 2.0 ** -8  # about sqrt(eps): see the module docstring
# Salt of the parameter seed of a shape, chosen so that every ambiguous-share cap holds (0 where absent).
# The caps are conditions on the recipe, not on the kernels: if another torch random stream tips a shape over
# 1 % (tests/test_bn_cases.py fails with "the data recipe does not suit this check"), re-pick its salt: try
# 0, 1, 2, ... and take the first with which test_recipe_preconditions, test_emulation_passes_every_assertion,
# test_pool_emulation_passes_and_its_mutants_fail and test_ambiguous_shares_of_the_recipes pass (for the small
# shapes prefer a salt with no ambiguous element at all), then update the shares in the docstring above.
SALT = {(2, 32, 1, 3): 1, (1, 48, 1, 1): 3, (2, 48, 29, 31): 1, (33, 32, 128, 128): 1}
SLOTS = 16  # kStatSlots of the f64 statistics workspace: [slot][2][C]

ALL_C = (32, 48, 64, 80, 96, 128, 160, 192, 256, 320, 384, 448, 512, 1024, 2048)
CHANNEL_SHAPES = [(3, c, 5, 7) for c in ALL_C]          # 105 rows: a multiple of neither RPI nor 4 * RPI
SMALL_SHAPES = [(2, 32, 1, 3), (1, 64, 1, 1), (1, 48, 1, 1)]  # rows < RPI; a single row
RAGGED_SHAPES = [(2, 32, 33, 33), (2, 48, 29, 31)]      # several chunks, a ragged last one
LARGE_SHAPES = [(33, 32, 128, 128), (11, 48, 128, 128)]  # chunk cap + grid cap; grid cap with 252 threads
UNIT_SHAPES = CHANNEL_SHAPES + SMALL_SHAPES + RAGGED_SHAPES
POOL_SHAPES = [(2, 64, 2, 2), (3, 32, 3, 2), (2, 64, 15, 17), (3, 128, 8, 8)]
MULTI_FWD = [(3, 48, 5, 7), (3, 192, 5, 7), (3, 320, 5, 7)]   # bn_finalize_multi: three BNs of different C
MULTI_BWD = [(3, 48, 5, 7), (3, 192, 5, 7), (3, 32, 5, 7)]    # bn_backward_multi: two narrower than the widest
# A full batch of kBnFinMax = 8 descriptors as (shape, rep): the shapes above repeated, every repeat with seeds
# of its own (rep > 0); the last BN of each batch is narrower than the widest.
MULTI8_FWD = [(s, i // 3) for i, s in enumerate((MULTI_FWD * 3)[:8])]
MULTI8_BWD = [(s, i // 3) for i, s in enumerate((MULTI_BWD[1:] + MULTI_BWD[:1]) * 3)][:8]


def seed_of(*key) -> int:
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def rows_of(shape) -> int:
    return shape[0] * shape[2] * shape[3]


def _ch(t):
    """A per-channel [C] tensor broadcast over NCHW, in float64."""
    return t.double().view(1, -1, 1, 1)


def _ints(shape, dense, name, hi, off, rep=0):
    seed = seed_of(name, shape, rep) if rep else seed_of(name, shape)
    if dense:
        return integer_data(shape, "dense", seed)
    return integer_data(shape, "ties", seed, hi=hi) - off


def make_case(shape, rep=0):
    """The CPU float32 inputs of one shape (NCHW; the GPU tests cast x / dy / res to bf16 channels_last);
    ``rep`` > 0: another draw of the same recipe (the repeated shapes of MULTI8_*).
    Cached, except for the two large shapes (0.2 GB each), which one test builds and drops."""
    return _build_case(shape, rep) if shape in LARGE_SHAPES else _cached_case(shape, rep)


def _build_case(shape, rep=0):
    N, C, H, W = shape
    dense = shape in LARGE_SHAPES
    salt = SALT.get((shape, rep) if rep else shape, 0)
    g = torch.Generator().manual_seed(seed_of("params", shape, salt, rep) if rep else seed_of("params", shape, salt))
    x = _ints(shape, dense, "x", 16, 7, rep)
    x[:, CONST_CH] = 1.0
    x[:, NEAR_CH] = 1.0
    x[N - 1, NEAR_CH, H - 1, W - 1] = 2.0
    gamma = torch.rand(C, generator=g) + 0.5
    gamma[::7] *= -1
    gamma[CONST_CH] = CONST_GAMMA
    if rows_of(shape) == 1:
        gamma *= GAMMA_SINGLE_ROW
    beta = torch.randn(C, generator=g) * 0.5
    beta[CONST_CH] = CONST_BETA
    c = {"shape": shape, "rows": rows_of(shape), "x": x, "dy": _ints(shape, dense, "dy", 8, 3, rep),
         "res": _ints(shape, dense, "res", 8, 4, rep), "dsx": _ints(shape, dense, "dsx", 8, 3, rep),
         "gamma": gamma, "beta": beta,
         "rm": torch.randn(C, generator=g) * 0.3, "rv": torch.rand(C, generator=g) + 0.5}
    # statistics the backward tests supply themselves (general f32 values, not the batch statistics of x)
    c["mean"] = torch.randn(C, generator=g) * 0.5
    c["invstd"] = torch.rand(C, generator=g) + 0.3
    c["fcoef"] = gate_coef(x, g)
    # the residual BN's coefficients of the res_coef variant
    c["rcoef"] = torch.cat([torch.rand(C, generator=g) * 0.5 + 0.25, torch.randn(C, generator=g) * 0.3])
    c["rcoef"][CONST_CH], c["rcoef"][C + CONST_CH] = 0.5, 0.5  # the constant channel stays on multiples of 1/4
    # ReLU mask bits unrelated to the gate of fcoef: a backward that ignored them would show
    c["mask"] = torch.randint(0, 256, (rows_of(shape) * C // 8,), dtype=torch.uint8, generator=g)
    return c


_cached_case = functools.lru_cache(maxsize=None)(_build_case)


def gate_coef(x, g):
    """Forward coefficients [scale; shift] for the backward's ReLU gate: general f32 values with every
    x * scale + shift (x an integer) at least 0.02 from 0, orders of magnitude beyond delta."""
    C = x.shape[1]
    sc = (torch.rand(C, generator=g) * 0.5 + 0.25) * torch.where(torch.arange(C) % 7 == 0, -1.0, 1.0)
    sh = torch.randn(C, generator=g) * 0.8
    for _ in range(64):
        pre = x.double() * _ch(sc) + _ch(sh)
        near = (pre.abs() < 0.02).flatten(2).any(2).any(0)
        if not near.any():
            break
        sh = torch.where(near, sh + 0.0437, sh)
    return torch.cat([sc, sh]).float()


def check_case(c):
    """The preconditions of a recipe, on the inputs alone: bf16-exact integers, exact f32 sums, the special
    channels, negative gammas, gates away from 0."""
    x, dy, res, rows = c["x"], c["dy"], c["res"], c["rows"]
    for name in ("x", "dy", "res", "dsx"):
        t = c[name]
        assert torch.equal(t, t.round()) and t.abs().max() <= 8, name
        assert torch.equal(t.bfloat16().float(), t), name
    xm, gm = x.abs().max().item(), 4 * dy.abs().max().item()  # the pool gradient gathers up to 4 windows
    # every per-chunk f32 sum of x, x^2, dz, dz * x is bounded by the whole-tensor sum of magnitudes
    for name, term in (("x", xm), ("x^2", xm * xm), ("dz", gm), ("dz*x", gm * xm)):
        assert rows * term < 2 ** 24, (c["shape"], name, rows * term)
    assert (x[:, CONST_CH] == 1).all()
    assert (x[:, NEAR_CH] != 1).sum().item() == 1 and x[-1, NEAR_CH, -1, -1] == 2
    scale = GAMMA_SINGLE_ROW if rows == 1 else 1.0
    assert (c["gamma"][::7] < 0).all() and (c["gamma"].abs() >= 0.5 * scale).all()
    assert not torch.equal(unpack_mask(c["mask"], rows, x.shape[1]).view(x.shape[0], x.shape[2], x.shape[3], -1)
                           .permute(0, 3, 1, 2), gate(x, c["fcoef"])[1])
    n_near, _ = gate(x, c["fcoef"])
    assert n_near == 0, "fcoef: %d gate arguments within delta of 0" % n_near


def split_slots(s64, q64, key):
    """The exact integer sums (s, q) spread unevenly over the SLOTS slots of a [SLOTS][2][C] f64 workspace:
    integer parts, so the kernel's f64 sum over the slots is exact in any order."""
    g = torch.Generator().manual_seed(seed_of("slots", key))
    C = s64.numel()
    ws = torch.zeros(SLOTS, 2, C, dtype=torch.float64, device=s64.device)
    for j, v in enumerate((s64, q64)):
        w = torch.rand(SLOTS, C, generator=g, dtype=torch.float64).to(v.device) ** 3
        w[3] = 0  # an empty slot
        part = torch.floor(v.abs() * w / w.sum(0)) * torch.sign(v)
        part[5] -= 17.0  # and slots of the opposite sign
        part[SLOTS - 1] += v - part.sum(0)
        ws[:, j] = part
    assert torch.equal(ws[:, 0].sum(0), s64) and torch.equal(ws[:, 1].sum(0), q64)
    return ws.reshape(-1)


# ---- forward: statistics and finalize -------------------------------------------------------------

def fwd_sums(x):
    xd = x.double()
    return xd.sum((0, 2, 3)), (xd * xd).sum((0, 2, 3))


def _ulps(got, ref, dtype=torch.float32):
    return ((got.double() - ref).abs() / ulp_of(ref, dtype)).max().item() if ref.numel() else 0.0


def _within(got, ref, delta, what):
    err = (got.double() - ref).abs()
    bad = ~(err <= delta)
    if bad.any():
        i = int(bad.nonzero()[0])
        raise AssertionError("%s: %d of %d channels off; first c=%d got %r expected %r (delta %.3g)" % (
            what, int(bad.sum()), bad.numel(), i, got[i].item(), ref[i].item(), delta[i].item()))


def _bits_f32(got, ref64, what):
    exp = ref64.float()
    bad = got != exp
    if bad.any():
        i = int(bad.nonzero()[0])
        raise AssertionError("%s: %d of %d channels differ; first c=%d got %r expected %r" % (
            what, int(bad.sum()), bad.numel(), i, got[i].item(), exp[i].item()))


def check_finalize(what, s, q, rows, gamma, beta, rm0, rv0, out, momentum=MOMENTUM, eps=EPS):
    """Training-mode finalize from the exact f64 sums (s, q).  ``out``: mean, invstd, coef, rm, rv, nbt0,
    nbt (the kernel's outputs, running statistics after the call, num_batches before / after)."""
    mean, invstd, coef, rm1, rv1, nbt0, nbt1 = out
    C = s.numel()
    m = s / rows
    var = (q / rows - m * m).clamp_min(0)
    _bits_f32(mean, m, what + " mean")
    eps32 = torch.tensor(eps, dtype=torch.float32).double().item()
    is_ref = 1.0 / torch.sqrt(var.float().double() + eps32)
    ul = _ulps(invstd, is_ref)
    assert ul <= INVSTD_ULPS, "%s invstd: %.1f f32 ulp from 1/sqrt(float32(var) + eps)" % (what, ul)
    # one multiply: the product of two f32 is exact in f64, .float() rounds it once
    _bits_f32(coef[:C], gamma.double() * invstd.double(), what + " scale")
    mf, sc = mean.double(), coef[:C].double()
    # shift = beta - float32(m) * scale: the product and the difference round (k = 2)
    _within(coef[C:], beta.double() - mf * sc, U * 2 * (beta.double().abs() + (mf * sc).abs()), what + " shift")
    mom = torch.tensor(momentum, dtype=torch.float32).double().item()
    # running stats: 1 - momentum, its product, momentum * value, the sum (k = 4; + float32(unbiased): 5)
    _within(rm1, (1 - mom) * rm0.double() + mom * mf,
            U * 4 * (((1 - mom) * rm0.double()).abs() + (mom * mf).abs()), what + " running_mean")
    unb = var * rows / (rows - 1) if rows > 1 else var
    _within(rv1, (1 - mom) * rv0.double() + mom * unb,
            U * 5 * (((1 - mom) * rv0.double()).abs() + (mom * unb).abs()), what + " running_var")
    assert int(nbt1) == int(nbt0) + 1, "%s: num_batches %d -> %d" % (what, int(nbt0), int(nbt1))


def check_eval_coef(what, gamma, beta, rm, rv, mean, invstd, coef, eps=EPS):
    """Eval-mode coefficients, from the running statistics alone."""
    C = gamma.numel()
    assert torch.equal(mean, rm), what + " mean"
    eps32 = torch.tensor(eps, dtype=torch.float32).double().item()
    ul = _ulps(invstd, 1.0 / torch.sqrt(rv.double() + eps32))
    assert ul <= INVSTD_ULPS, "%s invstd: %.1f ulp" % (what, ul)
    _bits_f32(coef[:C], gamma.double() * invstd.double(), what + " scale")
    t = rm.double() * gamma.double() * invstd.double()
    _within(coef[C:], beta.double() - t, U * 3 * (beta.double().abs() + t.abs()), what + " shift")  # 2 products, 1 sum


# ---- forward apply ---------------------------------------------------------------------------------

def fwd_ref(x, coef, res=None, rcoef=None):
    """(pre-activation value, delta) of y in float64 from the kernel's own f32 coefficients."""
    C = x.shape[1]
    a = x.double() * _ch(coef[:C])
    pre, mag, k = a + _ch(coef[C:]), a.abs() + _ch(coef[C:]).abs(), K_FWD
    if rcoef is not None:
        r = res.double() * _ch(rcoef[:C])
        pre, mag, k = pre + r + _ch(rcoef[C:]), mag + r.abs() + _ch(rcoef[C:]).abs(), K_FWD_RC
    elif res is not None:
        pre, mag = pre + res.double(), mag + res.double().abs()
    return pre, U * k * mag


def _nhwc_bits(mask, like):
    N, C, H, W = like.shape
    return unpack_mask(mask, N * H * W, C).view(N, H, W, C).permute(0, 3, 1, 2)


def check_fwd_apply(what, x, coef, y, relu, res=None, rcoef=None, mask=None):
    pre, delta = fwd_ref(x, coef, res, rcoef)
    assert_rounds_from(y, pre, delta, what + " y", relu=relu)
    if mask is not None:
        # bit k of a byte is the sign of the f32 value: that of the f64 value wherever |value| > delta
        sure = pre.abs() > delta
        bad = (_nhwc_bits(mask, x) != (pre > 0)) & sure
        n = int(bad.sum())
        assert n == 0, "%s mask: %d bits differ from the sign of the f64 value; first [n, c, h, w] = %s" % (
            what, n, bad.nonzero()[0].tolist())


# ---- backward --------------------------------------------------------------------------------------

def gate(x, fcoef):
    """(number of gate arguments within delta of 0, the gate x * scale + shift > 0 as bool) in float64."""
    pre, delta = fwd_ref(x, fcoef)
    return int((pre.abs() <= delta).sum()), pre > 0


def bwd_sums(dz, x):
    return dz.sum((0, 2, 3)), (dz * x.double()).sum((0, 2, 3))


def check_bwd_params(what, s0, s1, mean, invstd, dgamma, dbeta):
    """dbeta = sum dz bit for bit; dgamma = invstd * (sum dz * x - mean * sum dz) within 1 f32 ulp (the
    kernel's f64 difference may contract into an FMA)."""
    _bits_f32(dbeta, s0, what + " dbeta")
    ref = invstd.double() * (s1 - mean.double() * s0)
    ul = _ulps(dgamma, ref)
    assert ul <= 1.0, "%s dgamma: %.2f f32 ulp from the f64 formula" % (what, ul)


def bwd_ref(dz, x, rows, gamma, mean, invstd, dgamma, dbeta, training=True):
    """(dx, delta) in float64, the three coefficients rebuilt from the kernel's own dgamma / dbeta."""
    a = gamma.double() * invstd.double()
    if not training:
        t = _ch(a) * dz
        return t, U * K_BWD_EVAL * t.abs()
    k2 = -a * dgamma.double() * invstd.double() / rows
    ka, kb = -a * dbeta.double() / rows, k2 * mean.double()
    t1, t2 = _ch(a) * dz, _ch(k2) * x.double()
    ref = t1 + t2 + _ch(ka - kb)
    return ref, U * K_BWD * (t1.abs() + t2.abs() + _ch(ka.abs() + kb.abs()))


def check_bwd(what, c, dev, outs, relu, training=True, mask=None, want_dres=False, mean=None,
              invstd=None, fcoef=None, dy=None, sums=None):
    """dx, dres, dgamma, dbeta of one bn_backward call against the f64 reference of case ``c`` on ``dev``.
    ``sums``: the (sum dz, sum dz * x) the call was given in place of its own reduce pass."""
    dx, dres, dgamma, dbeta = outs
    x = c["x"].to(dev)
    dy = (c["dy"] if dy is None else dy).to(dev)
    mean = (c["mean"] if mean is None else mean).to(dev)
    invstd = (c["invstd"] if invstd is None else invstd).to(dev)
    if not relu:
        on = torch.ones_like(x, dtype=torch.bool)
    elif mask is not None:
        on = _nhwc_bits(mask, x)
    else:
        n_near, on = gate(x, (c["fcoef"] if fcoef is None else fcoef).to(dev))
        assert n_near == 0
    dz = dy.double() * on
    s0, s1 = bwd_sums(dz, x) if sums is None else sums
    check_bwd_params(what, s0, s1, mean, invstd, dgamma, dbeta)
    ref, delta = bwd_ref(dz, x, c["rows"], c["gamma"].to(dev), mean, invstd, dgamma, dbeta, training)
    assert_rounds_from(dx, ref, delta, what + " dx")
    if want_dres:
        assert_bits_equal(dres, dz, what + " dres")
    return dz


# ---- stem: BN + ReLU + MaxPool(3, 2, 1) ------------------------------------------------------------

def pool_out(n):
    return (n + 2 - 3) // 2 + 1


def windows(t, fill):
    """[9, N, C, OH, OW]: the 3x3 / stride 2 / pad 1 windows of NCHW ``t`` in scan order, ``fill`` outside."""
    N, C, H, W = t.shape
    OH, OW = pool_out(H), pool_out(W)
    p = torch.full((N, C, 2 * OH + 1, 2 * OW + 1), fill, dtype=t.dtype, device=t.device)
    p[:, :, 1:H + 1, 1:W + 1] = t
    return torch.stack([p[:, :, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2] for kh in range(3) for kw in range(3)])


def unpack_arg(arg, yp_shape):
    """The argmax bytes ([N, OH, OW, C]) as an int64 NCHW tensor."""
    N, C, OH, OW = yp_shape
    return arg.view(N, OH, OW, C).permute(0, 3, 1, 2).to(torch.int64)


def first_argmax(x, coef):
    """The f64 reference argmax (first position in scan order among exact ties) of relu(x * scale + shift)."""
    pre, _ = fwd_ref(x, coef)
    v = windows(pre.clamp_min(0), -1.0)
    eq = v == v.max(0).values
    order = torch.arange(9, 0, -1, device=x.device).view(9, 1, 1, 1, 1)
    return (eq * order).argmax(0)


def check_pool_fwd(what, x, coef, yp, arg, xarg):
    pre, delta = fwd_ref(x, coef)
    inside = windows(torch.ones_like(pre), 0.0) > 0
    a = unpack_arg(arg, yp.shape).unsqueeze(0)
    assert int(a.max()) <= 8 and inside.gather(0, a).all(), what + ": a reported position lies outside the image"
    wp, wd, wx = windows(pre, 0.0), windows(delta, 0.0), windows(x.double(), 0.0)
    assert_rounds_from(yp, wp.gather(0, a)[0], wd.gather(0, a)[0], what + " y", relu=True)
    if xarg is not None:
        assert_bits_equal(xarg, wx.gather(0, a)[0], what + " xarg")
    # no window element beats the reported one by more than the two values' uncertainty
    post = torch.where(inside, wp.clamp_min(0), torch.full_like(wp, -1.0))
    over = post - post.gather(0, a) - (wd + wd.gather(0, a))
    assert not (over > 0).any(), "%s: %d windows hold a larger element than the reported one" % (
        what, int((over > 0).any(0).sum()))
    # exact ties (the same x in the same channel gives the same f32 value): the first in scan order wins
    k = torch.arange(9, device=x.device).view(9, 1, 1, 1, 1)
    earlier = inside & (wx == wx.gather(0, a)) & (k < a)
    assert not earlier.any(), "%s: %d windows report a later position of an exact tie" % (what, int(earlier.any(0).sum()))
    # a window whose output is 0 holds only zeros after the ReLU: its first element inside the image wins
    first_in = (inside * torch.arange(9, 0, -1, device=x.device).view(9, 1, 1, 1, 1)).argmax(0)
    zero = yp == 0
    assert torch.equal(a[0][zero], first_in[zero]), what + ": an all-zero window does not report its first element"


def pool_gather(dyp, a, x_shape):
    """The f64 gradient at the BN output: every input pixel receives dy of the windows whose argmax it is."""
    N, C, H, W = x_shape
    OH, OW = dyp.shape[2], dyp.shape[3]
    p = torch.zeros((N, C, 2 * OH + 1, 2 * OW + 1), dtype=torch.float64, device=dyp.device)
    for kh in range(3):
        for kw in range(3):
            p[:, :, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2] += dyp.double() * (a == kh * 3 + kw)
    assert (p[:, :, 0] == 0).all() and (p[:, :, :, 0] == 0).all() and (p[:, :, H + 1:] == 0).all() and \
        (p[:, :, :, W + 1:] == 0).all()
    return p[:, :, 1:H + 1, 1:W + 1]


# ---- a plain-torch f32 / bf16 emulation of the kernels, with mutants ----------------------------------

MUTANTS = ("truncate", "next_group", "last_row", "stats_row", "biased_var", "no_eps", "mask_bit", "k3_term")


def _store_bf16(v, mutant):
    if mutant == "truncate":
        return (v.contiguous().view(torch.int32) & -65536).view(torch.float32).bfloat16()
    return v.bfloat16()


def _next_group(coef, parts, mutant):
    """The coefficients a lane of channel group cv + 1 holds (mutant "next_group")."""
    if mutant != "next_group":
        return coef
    C = coef.numel() // parts
    return torch.roll(coef.view(parts, C), -8, 1).reshape(-1)


def _drop_last_row(t, mutant):
    if mutant == "last_row":
        t = t.clone()
        t[-1, :, -1, -1] = 0  # the buffer's previous content
    return t


def emu_forward(c, relu, with_res=False, with_rcoef=False, mutant=None, stats_of=None):
    """bn_forward in training mode, operation by operation as bn.hip does it: f64 sums and mean / variance,
    f32 everywhere else, separate (uncontracted) f32 roundings.  Returns a dict of its outputs."""
    x, rows = c["x"], c["rows"]
    xs = x if stats_of is None else stats_of  # sums=: the statistics of another tensor than the one applied to
    if mutant == "stats_row":
        xs = xs.clone()
        xs[-1, :, -1, -1] = 0
    s, q = fwd_sums(xs)
    m = s / rows
    var = (q / rows - m * m).clamp_min(0)
    eps = torch.tensor(0.0 if mutant == "no_eps" else EPS, dtype=torch.float32)
    invstd = torch.rsqrt(var.float() + eps)
    mean = m.float()
    mom = torch.tensor(MOMENTUM, dtype=torch.float32)
    unb = var * rows / (rows - 1) if rows > 1 and mutant != "biased_var" else var
    rm1 = (1 - mom) * c["rm"] + mom * mean
    rv1 = (1 - mom) * c["rv"] + mom * unb.float()
    sc = c["gamma"] * invstd
    coef = torch.cat([sc, c["beta"] - mean * sc])
    C = x.shape[1]
    k = _next_group(coef, 2, mutant)
    ksc, ksh = k[:C].view(1, -1, 1, 1), k[C:].view(1, -1, 1, 1)
    mask = None
    if with_rcoef:
        rc = _next_group(c["rcoef"], 2, mutant)
        v = x * ksc + (ksh + rc[C:].view(1, -1, 1, 1))
        v = v + c["res"] * rc[:C].view(1, -1, 1, 1)
    else:
        v = x * ksc + ksh
        if with_res:
            v = v + c["res"]
    if relu:
        if with_res or with_rcoef:
            mask = pack_mask(v > 0)
            if mutant == "mask_bit":
                mask[mask.numel() // 2] ^= 4
        v = v.clamp_min(0)
    y = _drop_last_row(_store_bf16(v, mutant), mutant)
    return {"y": y, "mean": mean, "invstd": invstd, "coef": coef, "rm": rm1, "rv": rv1, "mask": mask, "s": s, "q": q}


def pack_mask(on):
    """bool NCHW -> the kernels' 1-bit mask bytes (bit k of byte j of a row = channel 8j + k)."""
    r = on.permute(0, 2, 3, 1).reshape(-1, on.shape[1])
    w = (r.view(r.shape[0], -1, 8).to(torch.int32) << torch.arange(8, dtype=torch.int32)).sum(-1)
    return w.to(torch.uint8).reshape(-1)


def emu_backward(c, relu, training=True, use_mask=False, mutant=None, dy=None, sums_of=None):
    """bn_backward with the case's own mean / invstd / fcoef (or a mask of the same gate); ``dy``: another
    gradient than the case's (the stem pool's gathered one)."""
    x, dy, rows = c["x"], c["dy"] if dy is None else dy, c["rows"]
    C = x.shape[1]
    mean, invstd, gamma = c["mean"], c["invstd"], c["gamma"]
    fc = c["fcoef"]
    if not relu:
        on = torch.ones_like(x, dtype=torch.bool)
    elif use_mask:
        on = _nhwc_bits(c["mask"], x)
    else:
        on = x * fc[:C].view(1, -1, 1, 1) + fc[C:].view(1, -1, 1, 1) > 0
    mask = c["mask"] if relu and use_mask else None
    if mutant == "mask_bit":
        # the gate of one element with a non-zero gradient
        i = tuple(dy.nonzero()[dy.nonzero().shape[0] // 2].tolist())
        on = on.clone()
        on[i] = ~on[i]
    g = dy * on
    gs = g if sums_of is None else sums_of * on  # sums=: the sums of another gradient than the one applied
    if mutant == "stats_row":
        gs = gs.clone()
        gs[-1, :, -1, -1] = 0
    s0, s1 = bwd_sums(gs.double(), x)
    dg = invstd.double() * (s1 - mean.double() * s0)
    dgamma, dbeta = dg.float(), s0.float()
    a = gamma * invstd
    if training:
        inv_m = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(rows), dtype=torch.float32)
        k2 = -a * dgamma * invstd * inv_m
        k3 = -a * dbeta * inv_m
        if mutant != "k3_term":
            k3 = k3 - k2 * mean
    else:
        k2, k3 = torch.zeros(C), torch.zeros(C)
    k = _next_group(torch.cat([a, k2, k3]), 3, mutant)
    v = k[:C].view(1, -1, 1, 1) * g + k[C:2 * C].view(1, -1, 1, 1) * x + k[2 * C:].view(1, -1, 1, 1)
    dx = _drop_last_row(_store_bf16(v, mutant), mutant)
    dres = _drop_last_row(g.bfloat16(), mutant)
    return {"dx": dx, "dres": dres, "dgamma": dgamma, "dbeta": dbeta, "mask": mask}


def emu_pool_forward(c, coef, mutant=None):
    """bn_pool_apply_kernel in f32: (y, argmax bytes, xarg).  Mutants: "last_tie" reports the last position
    of an exact tie, "unclipped" reports position 0 of every window, inside the image or not."""
    x = c["x"]
    C = x.shape[1]
    v = (x * coef[:C].view(1, -1, 1, 1) + coef[C:].view(1, -1, 1, 1)).clamp_min(0)
    w = windows(v, -1.0)
    eq = w == w.max(0).values
    order = torch.arange(9, 0, -1).view(9, 1, 1, 1, 1) if mutant != "last_tie" else torch.arange(1, 10).view(9, 1, 1, 1, 1)
    a = (eq * order).argmax(0)
    if mutant == "unclipped":
        a = torch.zeros_like(a)
    y = w.gather(0, a.unsqueeze(0))[0].bfloat16()
    xarg = windows(x, 0.0).gather(0, a.unsqueeze(0))[0].bfloat16()
    return y, a.permute(0, 2, 3, 1).contiguous().to(torch.uint8).reshape(-1), xarg
