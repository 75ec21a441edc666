"""CPU checks of kungfu_amd.utils.numerics, the f64 BN-gradient reference the model-level GPU test
(tests/test_gpu_engine.py::test_resnet50_bn_param_grads_match_f64_on_shared_inputs) pins the fused
BN-backward sums with: the reference equals torch autograd in f64, and the assertion helper rejects
a sign-flipped, a permuted and an unrelated gradient.

And of the bit-exact integer-data criterion the MFMA kernel tests use (tests/test_gpu_exact.py): the
tolerance criteria of the older tests accept a lost tap, truncation and a one-ulp error, the exact
criterion rejects all three, and every data recipe of the GPU tests meets its preconditions."""
import pytest
import torch
import torch.nn.functional as F

from kungfu_amd.utils.numerics import (assert_bits_equal, bn_param_grads_f64, check_bn_param_grads,
                                       check_exact_reference, integer_data, rel_err, tie_fraction, unpack_mask)


def _pack(on: torch.Tensor) -> torch.Tensor:
    """bool [rows, C] -> the kernels' 1-bit mask bytes (bit k of byte j = channel 8j + k)."""
    w = (on.view(on.shape[0], -1, 8).to(torch.int32) << torch.arange(8, dtype=torch.int32)).sum(-1)
    return w.to(torch.uint8).reshape(-1)


def _setup(seed, n=3, c=16, h=5, w=7):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, c, h, w, generator=g) * 1.7 + 0.4).bfloat16().float()
    gamma = torch.rand(c, generator=g, dtype=torch.float64) + 0.5
    beta = torch.randn(c, generator=g, dtype=torch.float64) * 0.3
    dz = torch.randn(n, c, h, w, generator=g).bfloat16().float()
    return x, gamma, beta, dz


def _stats(x):
    xd = x.double()
    mean = xd.mean((0, 2, 3))
    var = xd.var((0, 2, 3), unbiased=False)
    return mean, (var + 1e-5).rsqrt()


def test_relu_reference_matches_autograd_f64():
    x, gamma, beta, dz = _setup(1)
    gm, bt = gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    z = torch.relu(F.batch_norm(x.double(), None, None, gm, bt, training=True, eps=1e-5))
    z.backward(dz.double())
    mean, invstd = _stats(x)
    scale = (gamma * invstd).float()
    coef = torch.cat([scale, (beta - mean * gamma * invstd).float()])
    dg, db = bn_param_grads_f64(dz, x, mean, invstd, "relu", coef)
    assert rel_err(gm.grad, dg) < 1e-5 and rel_err(bt.grad, db) < 1e-5


def test_mask_and_plain_references_match_autograd_f64():
    x, gamma, beta, dz = _setup(2)
    res = torch.randn_like(x).double()
    gm, bt = gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    z = torch.relu(F.batch_norm(x.double(), None, None, gm, bt, training=True, eps=1e-5) + res)
    z.backward(dz.double())
    mean, invstd = _stats(x)
    on = (z > 0).permute(0, 2, 3, 1).reshape(-1, x.shape[1])
    mask = _pack(on)
    assert torch.equal(unpack_mask(mask, on.shape[0], on.shape[1]), on)
    dg, db = bn_param_grads_f64(dz, x, mean, invstd, "mask", mask)
    assert rel_err(gm.grad, dg) < 1e-5 and rel_err(bt.grad, db) < 1e-5
    # plain: the gradient at the BN output itself
    gm2, bt2 = gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    F.batch_norm(x.double(), None, None, gm2, bt2, training=True, eps=1e-5).backward(dz.double())
    dg2, db2 = bn_param_grads_f64(dz, x, mean, invstd, "plain")
    assert rel_err(gm2.grad, dg2) < 1e-5 and rel_err(bt2.grad, db2) < 1e-5


def test_check_rejects_flipped_permuted_and_unrelated_gradients():
    x, gamma, beta, dz = _setup(3, c=64)
    mean, invstd = _stats(x)
    ref = bn_param_grads_f64(dz, x, mean, invstd, "plain")
    assert check_bn_param_grads(ref, (ref[0].float(), ref[1].float())) is None
    assert check_bn_param_grads(ref, (ref[0] * (1 + 1e-5), ref[1])) is None
    flipped = check_bn_param_grads(ref, (-ref[0], ref[1]))
    assert flipped is not None and "dgamma" in flipped
    assert check_bn_param_grads(ref, (ref[0], -ref[1])) is not None
    perm = torch.randperm(ref[0].numel(), generator=torch.Generator().manual_seed(0))
    assert check_bn_param_grads(ref, (ref[0][perm], ref[1])) is not None
    other = torch.randn(ref[0].shape, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    assert check_bn_param_grads(ref, (other * ref[0].norm() / other.norm(), ref[1])) is not None
    # the r5 envelope this replaces: 2x a stock-bf16 relative error of ~1.3 accepts all of these
    assert rel_err(ref[0], -ref[0]) == 2.0


# ---- the bit-exact integer-data criterion ----------------------------------------------------------

def _max_rel(ref, got):
    return ((got.double() - ref).abs().max() / ref.abs().max()).item()


def _truncate_to_bf16(ref_f64):
    """f64 -> f32 -> bf16 by dropping the low 16 bits (round toward zero) instead of rounding to nearest even."""
    bits = ref_f64.float().contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32).bfloat16()


def _one_ulp_off(got_bf16, index):
    out = got_bf16.clone()
    flat = out.view(-1).view(torch.int16)
    flat[index] += 1
    return out


def _lose_centre_tap(x, w, ref, n, oh, ow):
    """The exact output with the centre tap of a 3x3 pad-1 conv missing at pixel (n, oh, ow), all channels."""
    out = ref.clone()
    out[n, :, oh, ow] -= w[:, :, 1, 1].double() @ x[n, :, oh, ow].double()
    return out


def test_integer_data_kinds_and_determinism():
    s = integer_data((64, 1024), "sparse", 3)
    assert set(s.unique().tolist()) == {-1.0, 0.0, 1.0}
    assert abs((s != 0).float().mean().item() - 0.25) < 0.01
    d = integer_data((64, 1024), "dense", 3)
    assert set(d.unique().tolist()) == {-2.0, -1.0, 1.0, 2.0}
    t = integer_data((64, 1024), "ties", 3, hi=6)
    assert set(t.unique().tolist()) == {0.0, 1.0, 2.0, 3.0, 4.0, 5.0}
    for kind in ("sparse", "dense", "ties"):
        a = integer_data((5, 7), kind, 11)
        assert torch.equal(a, integer_data((5, 7), kind, 11)) and a.dtype == torch.float32
        assert not torch.equal(integer_data((64, 64), kind, 11), integer_data((64, 64), kind, 12))
        assert torch.equal(a.bfloat16().float(), a)  # exact in bf16
    with pytest.raises(ValueError):
        integer_data((2,), "uniform", 0)


def test_tie_fraction_counts_exact_halfway_values():
    # bf16 spacing is 2 on [256, 512) and 4 on [512, 1024): 257 and 514 are ties; 258, 512 and 516 are not
    r = torch.tensor([257.0, 258.0, 256.0, 514.0, 516.0, 512.0, 3.0, -259.0], dtype=torch.float64)
    assert tie_fraction(r) == 3 / 8
    assert tie_fraction(torch.arange(0, 257, dtype=torch.float64)) == 0.0
    # a tie is where the rounding modes part: nearest-even goes to the even neighbour, truncation goes down
    assert torch.tensor([257.0, 259.0]).bfloat16().tolist() == [256.0, 260.0]
    assert _truncate_to_bf16(torch.tensor([257.0, 259.0], dtype=torch.float64)).tolist() == [256.0, 258.0]


def test_assert_bits_equal_enforces_preconditions_on_the_reference():
    ref = torch.tensor([[1.0, -2.0], [256.0, 0.0]], dtype=torch.float64)
    assert_bits_equal(ref.bfloat16(), ref, "ok")
    assert_bits_equal(ref.float(), ref, "ok f32")
    assert_bits_equal(torch.tensor([[1.0, -2.0], [256.0, -0.0]]).bfloat16(), ref, "signed zero")
    with pytest.raises(AssertionError, match="integer"):
        assert_bits_equal(ref.bfloat16(), ref + 0.5, "half")
    with pytest.raises(AssertionError, match="f32"):
        assert_bits_equal(ref.float(), ref * 2.0 ** 17, "big")
    with pytest.raises(AssertionError, match="bf16"):
        assert_bits_equal((ref + 1).bfloat16(), ref + 1, "257")
    assert_bits_equal((ref + 1).bfloat16(), ref + 1, "257 as a tie", ties=True)
    assert_bits_equal((ref + 1).float(), ref + 1, "257 in f32")
    with pytest.raises(AssertionError, match="shape"):
        assert_bits_equal(ref.bfloat16().view(-1), ref, "shape")
    with pytest.raises(AssertionError, match=r"1 of 4 elements.*\n.*\(1, 0\)  got 255.0  expected 256.0"):
        assert_bits_equal(torch.tensor([[1.0, -2.0], [255.0, 0.0]]).bfloat16(), ref, "named")
    with pytest.raises(AssertionError):
        assert_bits_equal(torch.tensor([[1.0, -2.0], [float("nan"), 0.0]]).bfloat16(), ref, "nan")
    with pytest.raises(AssertionError):
        check_exact_reference(ref.float(), torch.bfloat16)  # the reference itself must be float64


@pytest.fixture(scope="module")
def randn_conv():
    """The exact f64 3x3 conv of bf16-valued randn data at the size of the (2, 64, 56, 57) -> 64 GPU case."""
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 64, 56, 57, generator=g).bfloat16().float()
    w = (torch.randn(64, 64, 3, 3, generator=g) * 0.05).bfloat16().float()
    return x, w, F.conv2d(x.double(), w.double(), padding=1)


def test_tolerance_criteria_accept_the_injected_errors(randn_conv):
    """What the 1e-2 criteria of the randn tests let through: whole-tensor relative L2 accepts a pixel that
    lost its centre tap, truncation and a one-ulp error; max|err| / max|ref| accepts the last two."""
    x, w, ref = randn_conv
    clean = ref.float().bfloat16()
    assert rel_err(ref, clean) < 2.5e-3 and _max_rel(ref, clean) < 4e-3  # bf16 rounding alone
    lost = _lose_centre_tap(x, w, ref, 1, 20, 31).float().bfloat16()
    trunc = _truncate_to_bf16(ref)
    ulp = _one_ulp_off(clean, 12345)
    assert not torch.equal(lost, clean) and not torch.equal(trunc, clean) and not torch.equal(ulp, clean)
    for name, bad in (("lost tap", lost), ("truncation", trunc), ("one ulp", ulp)):
        assert rel_err(ref, bad) < 1e-2, name
    for name, bad in (("truncation", trunc), ("one ulp", ulp)):
        assert _max_rel(ref, bad) < 1e-2, name
    assert _max_rel(ref, lost) > 1e-2  # the one error of the three a max-relative test does see


def test_exact_criterion_rejects_the_injected_errors():
    """The same three injections on integer data: each one fails assert_bits_equal (truncation on ties data,
    where it differs from round-to-nearest-even)."""
    x = integer_data((2, 64, 9, 11), "dense", 1)
    w = integer_data((64, 64, 3, 3), "sparse", 2)
    ref = F.conv2d(x.double(), w.double(), padding=1)
    clean = ref.float().bfloat16()
    assert_bits_equal(clean, ref, "clean")
    assert (ref != 0).double().mean().item() > 0.9  # few zeros for an error to hide behind
    with pytest.raises(AssertionError, match=r"of 12672 elements differ.*\n  \(1, \d+, 4, 7\)"):
        assert_bits_equal(_lose_centre_tap(x, w, ref, 1, 4, 7).float().bfloat16(), ref, "lost tap")
    with pytest.raises(AssertionError, match="1 of 12672 elements differ"):
        assert_bits_equal(_one_ulp_off(clean, 4321), ref, "one ulp")
    # truncation leaves integers within 256 alone: it needs the ties recipe
    assert torch.equal(_truncate_to_bf16(ref), clean)
    xt = integer_data((2, 64, 9, 11), "ties", 3, hi=4)
    wt = integer_data((64, 64, 3, 3), "ties", 4, hi=2)
    rt = F.conv2d(xt.double(), wt.double(), padding=1)
    assert tie_fraction(rt) >= 0.10
    assert_bits_equal(rt.float().bfloat16(), rt, "clean ties", ties=True)
    with pytest.raises(AssertionError, match="elements differ"):
        assert_bits_equal(_truncate_to_bf16(rt), rt, "truncation", ties=True)


def test_exact_data_recipes_meet_their_preconditions():
    """Every recipe of tests/test_gpu_exact.py through its CPU f64 reference: integer-valued, exact in f32
    partial sums, within 256 for bf16 outputs (ties: at least 10 % exact ties instead), per-channel f32 sums
    below 2^24 -- so no precondition can fail first on the GPU."""
    import exact_cases

    n = 0
    for label, case in exact_cases.all_cases():
        for name, ref, dtype, ties in case["refs"]:
            check_exact_reference(ref, dtype, ties, "%s: %s" % (label, name))
            if ties:
                assert tie_fraction(ref) >= 0.10, (label, name, tie_fraction(ref))
            n += 1
        for name, rows, term in case["sums"]:
            assert rows * term < 2 ** 24, (label, name, rows, term)
    assert n > 200
