"""Shape tables, inputs and float64 references of the bit-exact tests of the 64-channel image stem
(csrc/kernels/stem3.hip at Cout 64: VGG-16's first layer, tests/test_gpu_image_conv.py), and the CPU check of
every recipe's preconditions, so none can fail first on the GPU.

Everything is built through tests/exact_cases.py (``conv_case``, ``wgrad_case``, ``stat_sums``): small-integer
operands whose products and f32 partial sums are exact, compared with torch in float64.  The bias is
``integer_data((64,), "dense", seed) * 4`` (values in {-8, -4, 4, 8}), added in float64 before the clamp."""
import functools

import exact_cases as X
from kungfu_amd.utils.numerics import check_exact_reference, integer_data, tie_fraction

COUT = 64
# (n, h, w, k, stride, pad); the last: M = 15, less than one 16-pixel MFMA tile
CASES = [(2, 29, 31, 3, 1, 1), (4, 20, 18, 2, 1, 0), (3, 9, 11, 3, 2, 1), (1, 5, 3, 3, 1, 1)]
TIES = ((2, 29, 31, 3, 1, 1), 48)  # case, hi: x in [0, 48), w in {0, 1}
# past the grid caps, so the grid-stride loops run more than once: the forward launches at most 2048 workgroups
# x 256 pixels (524288 pixels), the weight gradient 512 blocks x 256 pixels (131072 pixels)
FWD_GRID_CAP = 2048 * 256
WGRAD_GRID_CAP = 512 * 256
BIG_FWD = (11, 224, 224, 3, 1, 1)    # 551936 pixels; bias + ReLU, no statistics (rows * term >= 2^24 here)
BIG_WGRAD = (3, 224, 224, 3, 1, 1)   # 150528 pixels; f32 output only (the reference passes 256)


def out_hw(h, w, k, s, p):
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


@functools.lru_cache(maxsize=None)
def bias_of(key):
    return integer_data((COUT,), "dense", X.seed_of("image conv bias", key)) * 4


@functools.lru_cache(maxsize=None)
def fwd_case(n, h, w, k, s, p, kind="dense", hi=4, stats=True):
    """conv_case at Cout 64 plus the bias and bias + ReLU references (and the statistics of the plain output)."""
    oh, ow = out_hw(h, w, k, s, p)
    c = X.conv_case(n, h, w, 3, COUT, k, k, s, p, p, kind, hi)
    c = X.stat_sums(c, n * oh * ow) if stats else dict(c)
    ties = kind == "ties"
    c["bias"] = bias_of((n, h, w, k, s, p, kind, hi))
    c["with_bias"] = c["ref"] + c["bias"].double().view(1, -1, 1, 1)
    c["bias_relu"] = c["with_bias"].clamp_min(0)
    c["refs"] = list(c["refs"]) + [("y + bias", c["with_bias"], X.BF16, ties), ("relu(y + bias)", c["bias_relu"], X.BF16, ties)]
    return c


def wgrad_case(n, h, w, k, s, p):
    return X.wgrad_case(n, 3, h, w, COUT, k, k, s, p, p, "dense_x")


def ties_case():
    case, hi = TIES
    return fwd_case(*case, kind="ties", hi=hi, stats=False)


def big_fwd_case():
    return fwd_case(*BIG_FWD, stats=False)


def big_wgrad_case():
    return wgrad_case(*BIG_WGRAD)


def _check(label, case, only=None):
    n = 0
    for name, ref, dtype, ties in case["refs"]:
        if only is not None and name not in only:
            continue
        check_exact_reference(ref, dtype, ties, "%s: %s" % (label, name))
        if ties:
            assert tie_fraction(ref) >= 0.10, (label, name, tie_fraction(ref))
        n += 1
    for name, rows, term in case["sums"]:
        assert rows * term < 2 ** 24, (label, name, rows, term)
    return n


def test_forward_cases_meet_their_preconditions():
    n = 0
    for case in CASES:
        c = fwd_case(*case)
        n += _check("image conv fwd %r" % (case,), c)
        assert len(c["sums"]) == 2 and c["ref"].abs().max().item() <= 20
        assert c["bias_relu"].abs().max().item() <= 27
        assert set(c["bias"].abs().unique().tolist()) <= {4.0, 8.0}
    assert n == 3 * len(CASES)
    # both sides of the ReLU gate are exercised
    c = fwd_case(*CASES[0])
    clamped = (c["with_bias"] <= 0).double().mean().item()
    assert 0.25 < clamped < 0.75, clamped


def test_ties_case_meets_its_preconditions():
    c = ties_case()
    assert c["sums"] == []  # no statistics at these magnitudes
    assert _check("image conv ties", c) == 3
    assert tie_fraction(c["bias_relu"]) >= 0.10
    assert c["bias_relu"].abs().max().item() > 256  # past the exact-integer range of bf16: the rounding shows


def test_wgrad_cases_meet_their_preconditions():
    for case in CASES:
        g = wgrad_case(*case)
        assert _check("image conv wgrad %r" % (case,), g, only=("dw", "dw f32")) == 2
        assert g["ref"].abs().max().item() <= 111


def test_grid_stride_cases_pass_the_caps_and_stay_exact():
    n, h, w, k, s, p = BIG_FWD
    oh, ow = out_hw(h, w, k, s, p)
    assert n * oh * ow > FWD_GRID_CAP >= (n - 1) * oh * ow  # the smallest batch past the cap
    c = big_fwd_case()
    assert c["sums"] == []
    check_exact_reference(c["bias_relu"], X.BF16, False, "big fwd relu(y + bias)")
    n, h, w, k, s, p = BIG_WGRAD
    oh, ow = out_hw(h, w, k, s, p)
    assert n * oh * ow > WGRAD_GRID_CAP >= (n - 1) * oh * ow
    g = big_wgrad_case()
    check_exact_reference(g["ref"], X.F32, False, "big wgrad f32")
    assert g["ref"].abs().max().item() > 256  # why the bf16 output is not compared at this size
