"""CPU checks of tests/rounding_cases.py (the recipe behind tests/test_gpu_conv_rounding.py) and of the conv
kernels' reciprocal division (csrc/kernels/recip_div.hpp, through build/recip_div_check):
  * every rounding case holds at least 64 output elements of every class, in both signs;
  * its reference (torch's CPU rounding of the exact f32 sum) equals the integer formula the kernels used
    before (common.hpp f32_to_bf16), so both rounding paths are held to the same bits;
  * the gather reference equals a float32 torch convolution on the addressing data;
  * the reciprocal division equals `//` for every divisor 1..32768 at the extreme and boundary dividends."""
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rounding_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (N, H, W) of the GPU rounding cases, output channels
ROUNDING_SHAPES = [(2, 8, 8), (2, 9, 9)]
COUTS = [64, 128, 256]


@pytest.mark.parametrize("shape", ROUNDING_SHAPES)
@pytest.mark.parametrize("cout", COUTS)
def test_every_class_is_present(shape, cout):
    x = R.rounding_input(*shape)
    assert not torch.isnan(x.float()).any() and not torch.isinf(x.float()).any()
    for ks in (1, 3):
        v = R.conv_sum(x, cout, ks)
        counts = {k: int(m.sum()) for k, m in R.classify(v).items()}
        for cls in R.CLASSES:
            for sg in ("_pos", "_neg"):
                if cls == "zero":
                    continue
                assert counts[cls + sg] >= R.MIN_PER_CLASS, (cls + sg, counts)
        # (-0, -0) inputs exist, and like (+0, +0) they sum to +0 on an accumulator that starts at +0
        bits = R.to_bits(x.permute(0, 2, 3, 1).reshape(-1, R.CIN))
        neg0 = ((bits[:, 0::2] == 0x8000) & (bits[:, 1::2] == 0x8000)).sum().item() * (cout // 32)
        pos0 = ((bits[:, 0::2] == 0) & (bits[:, 1::2] == 0)).sum().item() * (cout // 32)
        assert neg0 >= R.MIN_PER_CLASS and pos0 >= R.MIN_PER_CLASS
        assert counts["zero_pos"] >= neg0 + pos0 and counts["zero_neg"] == 0


@pytest.mark.parametrize("shape", ROUNDING_SHAPES)
def test_reference_equals_the_integer_formula(shape):
    x = R.rounding_input(*shape)
    v = R.conv_sum(x, 64, 1)
    assert not torch.isnan(v).any()
    assert torch.equal(R.to_bits(v.bfloat16()), R.round_int(v))
    # the sum is exact: float64 addition gives the same value (overflow to inf aside)
    xd = x.double()
    exact = xd[:, 0::2] + xd[:, 1::2]
    fin = torch.isfinite(v[:, :32])
    assert torch.equal(v[:, :32].double()[fin], exact[fin])


def test_integer_formula_one_ulp_from_a_tie_and_nan():
    """What two bf16 terms cannot form (rounding_cases docstring): low bits 0x7fff / 0x8001, on the f32 bit
    patterns themselves; and the NaN patterns the integer formula loses while torch keeps them NaN."""
    hi = torch.arange(0x0080, 0x7f7f, 37, dtype=torch.int64)
    hi = torch.cat([hi, hi | 0x8000])
    for low, up in ((0x7fff, 0), (0x8001, 1)):
        u = (hi << 16) | low
        v = torch.from_numpy(u.numpy().astype(np.uint32).view(np.float32).copy())
        want = (hi + up).to(torch.int32)
        assert torch.equal(R.round_int(v), want)
        assert torch.equal(R.to_bits(v.bfloat16()), want)
    nan = torch.from_numpy(np.array([0x7f800001, 0x7fffffff, 0xffffffff, 0x7fc00000], dtype=np.uint32).view(np.float32).copy())
    assert torch.isnan(nan.bfloat16().float()).all()
    got = R.round_int(nan).tolist()
    assert got[0] == 0x7f80 and got[1] == 0x8000 and got[2] == 0x0000  # +inf, -0, +0: not NaN


def test_one_ulp_recipe_is_exact_in_f32():
    """The bias case's three-term sums sit one f32 ulp either side of a tie, exactly (float64 agrees)."""
    x, bias = R.one_ulp_input(2, 9, 9), R.one_ulp_bias(128)
    s = R.conv_sum(x, 128, 1) + bias.float().view(1, -1, 1, 1)
    xd = x.double()
    exact = (xd[:, 0::2] + xd[:, 1::2]).repeat(1, 4, 1, 1) + bias.double().view(1, -1, 1, 1)
    assert torch.equal(s.double(), exact)
    low = s.contiguous().view(torch.int32) & 0xffff
    assert (low == 0x8001).sum() >= R.MIN_PER_CLASS and (low == 0x7fff).sum() >= R.MIN_PER_CLASS
    assert torch.equal(R.to_bits(s.bfloat16()), R.round_int(s))


@pytest.mark.parametrize("ks,stride,centre", [(1, 1, True), (3, 1, False), (1, 2, True), (3, 1, True)])
def test_gather_reference_equals_torch_conv(ks, stride, centre):
    x = R.position_input(3, 7, 11)
    w = R.weights(128, ks, centre)
    want = F.conv2d(x.float(), w.float(), stride=stride, padding=(ks - 1) // 2)
    got = R.conv_sum(x, 128, ks, stride, centre)
    assert torch.equal(got, want)
    assert torch.equal(got.bfloat16().float(), got)  # small integers: exact in bf16


def test_nan_input_has_nans_on_its_own_pixels():
    x = R.nan_input(2, 9, 9)
    nan_pix = torch.isnan(x.float()).any(1).reshape(-1)
    assert nan_pix.sum().item() == len(range(0, 162, 5)) and nan_pix[::5].all()


def test_reciprocal_division_equals_floor_division():
    subprocess.check_call(["make", "-C", ROOT, "-s", "build/recip_div_check"])
    r = subprocess.run([ROOT + "/build/recip_div_check"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout[-400:]
    seen = set()
    for line in r.stdout.splitlines():
        f = line.split()
        d, magic, shift = int(f[0]), int(f[1]), int(f[2])
        seen.add(d)
        L = (d - 1).bit_length()  # ceil(log2 d)
        assert shift == L and magic == (1 << (31 + L)) // d + 1 and magic < 1 << 32
        for nq in f[3:]:
            n, q = map(int, nq.split(":"))
            assert q == n // d, (n, d, q)
            assert ((2 * n * magic) >> 32) >> shift == q  # the formula, in unbounded integers
        for n in (2**31 - 1, 2**31 - d, (2**31 - 1) // d * d, (2**31 - 1) // d * d - 1):
            if 0 <= n < 2**31:
                assert ((2 * n * magic) >> 32) >> shift == n // d, (n, d)
    assert set(range(1, 32769)) <= seen
