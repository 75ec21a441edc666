"""CPU checks of the element-wise BatchNorm criterion (tests/bn_cases.py, kungfu_amd.utils.numerics.
assert_rounds_from) that tests/test_gpu_bn_exact.py applies to the kernels of csrc/kernels/bn.hip: every
recipe meets its preconditions, a plain-torch f32 / bf16 emulation of each stage passes the same assertions
(the positive control), and eight mutants of that emulation each fail them.

What `_rel(a, b) = max|a - b| / max|b| < 3e-2` (tests/test_gpu.py::test_fused_bn) makes of the same mutants,
measured here on the (3, 48, 5, 7) and (2, 32, 33, 33) recipes against the unmutated emulation and asserted
in test_what_the_3e_2_criterion_accepts:

  mutant       what it does                                       new assertions      _rel < 3e-2
  -----------  -------------------------------------------------  ------------------  ---------------------------
  truncate     bf16 store drops the low 16 bits                   fail (y, dx)        accepts
  next_group   lanes hold the coefficients of channel group + 1   fail (y, dx)        rejects: these recipes have
                                                                                      no small channels to hide in
  last_row     the last row of y / dx / dres is not written       fail (y, dx, dres)  rejects: integer data puts
                                                                                      large values in every row
  stats_row    one row missing from the sums                      fail (mean, dbeta)  forward: accepts; backward:
                                                                                      rejects at 105 rows, accepts
                                                                                      at 2178
  biased_var   running_var from the biased variance               fail (running_var)  accepts
  no_eps       eps dropped from invstd                            fail (invstd)       rejects, through the constant
                                                                                      channel's infinite invstd only
  mask_bit     one ReLU mask / gate bit flipped                   fail (mask; dbeta,  forward mask: accepts (never
                                                                  dres)               compared); backward: rejects,
                                                                                      the element is an integer
  k3_term      k3 without k2 * mean                               fail (dx)           rejects: the supplied mean
                                                                                      is not small

(The table's last column is what EXPECT_REL records, outcome by outcome.)"""
import pytest
import torch

import bn_cases as B
from kungfu_amd.utils.numerics import assert_rounds_from, round_to, rounding_interval, ulp_of

BF16 = torch.bfloat16
FWD_VARIANTS = [("plain", False, False, False), ("relu", True, False, False), ("res", False, True, False),
                ("res_relu", True, True, False), ("res_coef", True, False, True)]
BWD_VARIANTS = [("plain", False, True, False), ("relu_coef", True, True, False), ("relu_bits", True, True, True),
                ("eval", True, False, False)]


# ---- the helper ------------------------------------------------------------------------------------

def test_round_to_is_one_rounding_to_nearest_even():
    v = torch.tensor([1.0, 1.00390625, 1.01171875, 257.0, 259.0, -257.0, 0.0, 3.0e-39, 1.0 + 2.0 ** -8 + 2.0 ** -30],
                     dtype=torch.float64)
    # 1 + 2^-8 and 1 + 3 * 2^-8 are bf16 ties (spacing 2^-7): to even; the last is just above a tie
    assert round_to(v, BF16).tolist() == [1.0, 1.0, 1.015625, 256.0, 260.0, -256.0, 0.0,
                                          round_to(v[7:8], BF16).item(), 1.0078125]
    # ... which the double rounding through f32 lands on the tie and sends down
    assert v[8:].float().bfloat16().item() == 1.0
    g = torch.Generator().manual_seed(3)
    r = torch.randn(20000, generator=g, dtype=torch.float64) * torch.exp2(torch.randint(-20, 20, (20000,), generator=g))
    assert torch.equal(round_to(r, torch.float32), r.float().double())  # f64 -> f32 is one rounding in torch too
    exact = r.float().double()  # from an f32 value the bf16 conversion is a single rounding as well
    assert torch.equal(round_to(exact, BF16), exact.float().bfloat16().double())
    assert ulp_of(torch.tensor([1.0, 1.5, 2.0, 0.0], dtype=torch.float64), BF16).tolist()[:3] == [2.0 ** -7] * 2 + [2.0 ** -6]


def test_assert_rounds_from_accepts_the_neighbours_only_where_ambiguous():
    ref = torch.tensor([[1.0 + 2.0 ** -8 + 1e-9, 1.25, -3.0, 1e-3]], dtype=torch.float64)  # first: just above a tie
    delta = torch.full_like(ref, 1e-6)
    up = torch.tensor([[1.0078125, 1.25, -3.0, 1e-3]]).bfloat16()
    down = torch.tensor([[1.0, 1.25, -3.0, 1e-3]]).bfloat16()
    amb = assert_rounds_from(up, ref, delta, "up", max_ambiguous=0.25)
    assert amb.tolist() == [[True, False, False, False]]
    assert_rounds_from(down, ref, delta, "down", max_ambiguous=0.25)  # the other neighbour: ambiguous, accepted
    with pytest.raises(AssertionError, match="ambiguous"):
        assert_rounds_from(up, ref, delta, "cap")  # 25 % > 1 %: a condition on the recipe
    with pytest.raises(AssertionError, match=r"1 of 4 elements.*\n  \(0, 0\)  got 1.0  expected 1.0078125"):
        assert_rounds_from(down, ref, 0.0, "exact")  # without the uncertainty only RNE(ref) passes
    two_up = torch.tensor([[1.015625, 1.25, -3.0, 1e-3]]).bfloat16()
    with pytest.raises(AssertionError, match=r"got 1.015625  expected 1.0\.\.1.0078125"):
        assert_rounds_from(two_up, ref, delta, "two up", max_ambiguous=0.25)
    off = torch.tensor([[1.0, 1.2578125, -3.0, 1e-3]]).bfloat16()
    with pytest.raises(AssertionError, match=r"\(0, 1\)  got 1.2578125  expected 1.25"):
        assert_rounds_from(off, ref, delta, "one ulp", max_ambiguous=0.25)
    # ReLU: with 0 inside the interval, 0 or the neighbour; a negative output never
    pre = torch.tensor([[1e-7, -1e-7, -2.0, 2.0]], dtype=torch.float64)
    z = torch.tensor([[0.0, 0.0, 0.0, 2.0]]).bfloat16()
    assert assert_rounds_from(z, pre, delta, "relu", 0.5, relu=True).tolist() == [[True, True, False, False]]
    assert_rounds_from(torch.tensor([[1e-7, 5e-7, 0.0, 2.0]]).bfloat16(), pre, delta, "relu", 0.5, relu=True)
    with pytest.raises(AssertionError, match="not the rounded reference"):
        assert_rounds_from(torch.tensor([[-1e-7, 0.0, 0.0, 2.0]]).bfloat16(), pre, delta, "relu", 0.5, relu=True)
    with pytest.raises(AssertionError):
        assert_rounds_from(torch.tensor([[float("nan"), 0.0, 0.0, 2.0]]).bfloat16(), pre, delta, "nan", 0.5, relu=True)
    with pytest.raises(AssertionError, match="float64"):
        assert_rounds_from(z, pre.float(), delta, "f32 reference")
    # f32 outputs
    r32 = torch.tensor([1.0 + 2.0 ** -24 + 1e-12, 0.3], dtype=torch.float64)
    assert_rounds_from(r32.float(), r32, 1e-10, "f32", 0.5)
    with pytest.raises(AssertionError):
        assert_rounds_from(torch.tensor([1.0 + 2.0 ** -22, 0.3]), r32, 1e-10, "f32 off", 0.5)


def test_double_rounding_hides_ambiguous_elements():
    """ref -> f32 -> bf16 collapses ref +- delta onto one f32 value wherever delta is below the f32 spacing:
    it reports no ambiguous element where the f64 computation finds them."""
    g = torch.Generator().manual_seed(5)
    ref = torch.randn(1 << 18, generator=g, dtype=torch.float64) * 3
    ref[:64] = ref[:64].abs() + 1
    ref[:64] = round_to(ref[:64], BF16) + ulp_of(ref[:64], BF16) / 2 + 1e-9  # just above a tie
    delta = ref.abs() * 2.0 ** -26
    delta[:64] = 2e-9  # the interval holds the tie; both of its ends round to the tie's own f32 value
    amb = rounding_interval(ref, delta, BF16)[2]
    naive = (ref - delta).float().bfloat16() != (ref + delta).float().bfloat16()
    assert int(amb.sum()) >= 64 and int(naive.sum()) < int(amb.sum())
    assert not naive[:64].any() and amb[:64].all()


# ---- the recipes -------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", B.UNIT_SHAPES + B.POOL_SHAPES + B.LARGE_SHAPES, ids=str)
def test_recipe_preconditions(shape):
    B.check_case(B.make_case(shape))


def _fwd_out(c, e):
    return e["mean"], e["invstd"], e["coef"], e["rm"], e["rv"], 0, 1


def _check_fwd(c, e, relu, res, rc, stats_of=None):
    B.check_finalize("emu", *B.fwd_sums(c["x"] if stats_of is None else stats_of), c["rows"], c["gamma"], c["beta"],
                     c["rm"], c["rv"], _fwd_out(c, e))
    B.check_fwd_apply("emu", c["x"], e["coef"], e["y"], relu, c["res"] if (res or rc) else None,
                      c["rcoef"] if rc else None, e["mask"])


def _check_bwd(c, e, relu, training, bits, sums=None):
    B.check_bwd("emu", c, "cpu", (e["dx"], e["dres"], e["dgamma"], e["dbeta"]), relu, training,
                c["mask"] if bits else None, True, sums=sums)


@pytest.mark.parametrize("shape", B.UNIT_SHAPES, ids=str)
def test_emulation_passes_every_assertion(shape):
    """The positive control: the plain-torch emulation of every stage and variant through the assertions the
    kernels get, with the ambiguous-share cap of every recipe."""
    c = B.make_case(shape)
    n = 0
    for _, relu, res, rc in FWD_VARIANTS:
        _check_fwd(c, B.emu_forward(c, relu, res, rc), relu, res, rc)
        n += 1
    for relu in (False, True):  # sums=: the statistics of another tensor than the one normalised
        _check_fwd(c, B.emu_forward(c, relu, stats_of=c["dsx"]), relu, False, False, c["dsx"])
        n += 1
    for _, relu, training, bits in BWD_VARIANTS:
        _check_bwd(c, B.emu_backward(c, relu, training, bits), relu, training, bits)
        n += 1
    on = B.gate(c["x"], c["fcoef"])[1]
    _check_bwd(c, B.emu_backward(c, True, sums_of=c["res"]), True, True, False,
               B.bwd_sums(c["res"].double() * on, c["x"]))
    assert n + 1 == 12


@pytest.mark.parametrize("shape,rep", sorted(set(B.MULTI8_FWD + B.MULTI8_BWD)), ids=str)
def test_recipes_of_the_full_batches(shape, rep):
    """The recipes of the eight-BN batches (the repeats are draws of their own): the preconditions, and the
    emulation through the assertions their GPU tests apply, with the ambiguous-share cap."""
    c = B.make_case(shape, rep)
    B.check_case(c)
    _check_fwd(c, B.emu_forward(c, True, stats_of=c["dsx"]), True, False, False, c["dsx"])
    _check_bwd(c, B.emu_backward(c, True), True, True, False)


@pytest.mark.parametrize("shape", B.POOL_SHAPES, ids=str)
def test_pool_emulation_passes_and_its_mutants_fail(shape):
    """The stem pool's assertions on an f32 emulation: the clean one passes (forward, and the backward of the
    gathered gradient); reporting the last of an exact tie, or a position outside the image, fails."""
    c = B.make_case(shape)
    coef = B.emu_forward(c, True)["coef"]
    B.check_pool_fwd("emu", c["x"], coef, *B.emu_pool_forward(c, coef))
    for mutant, msg in (("last_tie", "later position of an exact tie"), ("unclipped", "outside the image")):
        with pytest.raises(AssertionError, match=msg):
            B.check_pool_fwd(mutant, c["x"], coef, *B.emu_pool_forward(c, coef, mutant))
    a = B.first_argmax(c["x"], c["fcoef"])
    dyp = B._ints((shape[0], shape[1], a.shape[2], a.shape[3]), False, "dyp", 8, 3)
    dyfull = B.pool_gather(dyp, a, shape)
    assert dyfull.sum().item() == dyp.double().sum().item()  # every window hands its gradient to one pixel
    e = B.emu_backward(c, True, dy=dyfull.float())
    B.check_bwd("emu pool", c, "cpu", (e["dx"], None, e["dgamma"], e["dbeta"]), True, dy=dyfull)


def test_ambiguous_shares_of_the_recipes():
    """The largest ambiguous share per kind (the figures of the bn_cases docstring), each below the 1 % cap; the
    two large shapes in the two variants they run in."""
    worst = {"fwd": 0.0, "bwd": 0.0}
    for shape in B.UNIT_SHAPES + B.LARGE_SHAPES:
        c = B.make_case(shape)
        large = shape in B.LARGE_SHAPES
        for name, relu, res, rc in FWD_VARIANTS:
            if large and name != "relu":
                continue
            e = B.emu_forward(c, relu, res, rc)
            pre, d = B.fwd_ref(c["x"], e["coef"], c["res"] if (res or rc) else None, c["rcoef"] if rc else None)
            worst["fwd"] = max(worst["fwd"], rounding_interval(pre, d, BF16, relu)[2].double().mean().item())
        for name, relu, training, bits in BWD_VARIANTS:
            if large and name != "relu_coef":
                continue
            e = B.emu_backward(c, relu, training, bits)
            on = B.gate(c["x"], c["fcoef"])[1] if relu else torch.ones_like(c["x"], dtype=torch.bool)
            on = B._nhwc_bits(c["mask"], c["x"]) if bits else on
            ref, d = B.bwd_ref(c["dy"].double() * on, c["x"], c["rows"], c["gamma"], c["mean"], c["invstd"],
                               e["dgamma"], e["dbeta"], training)
            worst["bwd"] = max(worst["bwd"], rounding_interval(ref, d, BF16)[2].double().mean().item())
    print("largest ambiguous shares:", worst)
    assert 0 < worst["fwd"] <= 0.01 and 0 < worst["bwd"] <= 0.01, worst  # the bn_cases docstring records them


# ---- the mutants -------------------------------------------------------------------------------------

MUTANT_SHAPES = [(3, 48, 5, 7), (2, 32, 33, 33)]


def _rel(a, b):
    return ((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-12)).item()


def _rel_catches(clean, bad, keys):
    worst = 0.0
    for k in keys:
        r = _rel(bad[k], clean[k])
        worst = max(worst, r if r == r else float("inf"))
    return worst >= 3e-2


def _fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


FWD_KEYS = ("y", "rm", "rv")
BWD_KEYS = ("dx", "dres", "dgamma", "dbeta")
# (mutant, stage): does `_rel < 3e-2` reject it, on MUTANT_SHAPES[0] (105 rows) and [1] (2178 rows)
EXPECT_REL = {("truncate", "fwd"): (False, False), ("truncate", "bwd"): (False, False),
              ("next_group", "fwd"): (True, True), ("next_group", "bwd"): (True, True),
              ("last_row", "fwd"): (True, True), ("last_row", "bwd"): (True, True),
              ("stats_row", "fwd"): (False, False), ("stats_row", "bwd"): (True, False),
              ("biased_var", "fwd"): (False, False),
              ("no_eps", "fwd"): (True, True),
              ("mask_bit", "fwd"): (False, False), ("mask_bit", "bwd"): (True, True),
              ("k3_term", "bwd"): (True, True)}


@pytest.mark.parametrize("mutant", B.MUTANTS)
def test_every_mutant_fails_the_new_assertions(mutant):
    for shape in MUTANT_SHAPES:
        c = B.make_case(shape)
        hit = 0
        if (mutant, "fwd") in EXPECT_REL:
            assert _fails(lambda: _check_fwd(c, B.emu_forward(c, True, True, False, mutant), True, True, False)), \
                (mutant, shape, "forward")
            hit += 1
        if (mutant, "bwd") in EXPECT_REL:
            assert _fails(lambda: _check_bwd(c, B.emu_backward(c, True, True, False, mutant), True, True, False)), \
                (mutant, shape, "backward")
            hit += 1
        assert hit >= 1


def test_what_the_3e_2_criterion_accepts():
    """EXPECT_REL, outcome by outcome: whether max|err| / max|ref| < 3e-2 on y / dx / dgamma / dbeta / running
    stats rejects each mutant (against the unmutated emulation, the most favourable reference there is)."""
    seen = {}
    for i, shape in enumerate(MUTANT_SHAPES):
        c = B.make_case(shape)
        cf, cb = B.emu_forward(c, True, True, False), B.emu_backward(c, True, True, False)
        for (mutant, stage) in EXPECT_REL:
            if stage == "fwd":
                got = _rel_catches(cf, B.emu_forward(c, True, True, False, mutant), FWD_KEYS)
            else:
                got = _rel_catches(cb, B.emu_backward(c, True, True, False, mutant), BWD_KEYS)
            seen.setdefault((mutant, stage), [None, None])[i] = got
    seen = {k: tuple(v) for k, v in seen.items()}
    assert seen == EXPECT_REL, {k: (seen[k], EXPECT_REL[k]) for k in seen if seen[k] != EXPECT_REL[k]}
    accepted = {k[0] for k, v in seen.items() if not all(v)}
    assert accepted == {"truncate", "stats_row", "biased_var", "mask_bit"}  # pass the old criterion at some shape
