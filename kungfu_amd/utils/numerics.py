"""Float64 references for checking fused kernels at model level.

:func:`bn_param_grads_f64` recomputes a BatchNorm's (dgamma, dbeta) in float64 from the SAME bf16
tensors the fused backward consumed: the BN input x, the gradient reaching the BN(+ReLU) output, the
batch mean / invstd and the ReLU gate.  Both sides then share every rounding up to the final
reduction, so the check can be tight (relative error ~1e-5) where a comparison against an f32 model
cannot: at random init the BN gamma/beta gradients are sums with massive cancellation, and bf16 vs
f32 differ in them by a relative error of 1.1-1.5 (profiles/r5_engine_numerics.md), a bound a
sign-flipped gradient would also meet.

No reference counterpart: the reference checks accuracy at the end of training
(``tests/python/integration/test_mnist_slp.py:149-165``), a regime this replaces for the fused
kernels with a per-parameter pin.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch


def unpack_mask(mask: torch.Tensor, rows: int, channels: int) -> torch.Tensor:
    """The fused kernels' 1-bit ReLU mask (one byte per 8 channels of an NHWC row, bit k = channel
    8j + k) as a bool [rows, channels] tensor."""
    bits = (mask.view(-1, 1).to(torch.int32) >> torch.arange(8, device=mask.device, dtype=torch.int32)) & 1
    return bits.view(rows, channels).bool()


def _rows(t: torch.Tensor) -> torch.Tensor:
    """[N, C, H, W] channels_last (or [rows, C]) -> [rows, C] in NHWC element order."""
    if t.dim() == 4:
        return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])
    return t.reshape(-1, t.shape[-1])


def bn_param_grads_f64(dz: torch.Tensor, x: torch.Tensor, mean: torch.Tensor, invstd: torch.Tensor,
                       kind: str, gate: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dgamma, dbeta) in float64 of ``z = act(gamma * (x - mean) * invstd + beta)``.

    ``kind``: ``"relu"`` -- act = ReLU, ``gate`` = the forward coefficients [scale(C); shift(C)]
    (relu' recomputed as x * scale + shift > 0, as the kernels do with one f32 FMA: its sign is the
    sign of the exact value, computed here in f64 -- x is bf16, so x * scale is exact in f64 and the
    one rounding of the sum keeps its sign; a separately rounded f32 product flips gates of
    elements whose BN output rounds to about zero); ``"mask"`` -- the
    ReLU gate is the 1-bit mask ``gate`` (a BN + residual + ReLU tail); ``"plain"`` -- no
    activation (``dz`` already is the gradient at the BN output)."""
    xr, dr = _rows(x), _rows(dz).double()
    C = xr.shape[1]
    if kind == "relu":
        sc, sh = gate[:C].float().double(), gate[C:2 * C].float().double()
        on = xr.double() * sc + sh > 0
        dr = dr * on
    elif kind == "mask":
        dr = dr * unpack_mask(gate, xr.shape[0], C)
    elif kind != "plain":
        raise ValueError(kind)
    xhat = (xr.double() - mean.double()) * invstd.double()
    return (dr * xhat).sum(0), dr.sum(0)


def rel_err(ref: torch.Tensor, got: torch.Tensor) -> float:
    """||got - ref|| / ||ref|| in float64 (0 when both are zero)."""
    ref, got = ref.double().reshape(-1), got.double().reshape(-1)
    n = ref.norm().item()
    d = (got - ref).norm().item()
    return d / n if n > 0 else d


def check_bn_param_grads(ref: Tuple[torch.Tensor, torch.Tensor], got: Tuple[torch.Tensor, torch.Tensor],
                         tol: float = 1e-3) -> Optional[str]:
    """None if both of ``got``'s (dgamma, dbeta) are within ``tol`` relative L2 error of ``ref``;
    otherwise a message naming the worse one.  A sign-flipped, permuted or unrelated gradient of the
    same norm scores 2, ~1.4 and ~1.4."""
    for name, r, g in (("dgamma", ref[0], got[0]), ("dbeta", ref[1], got[1])):
        e = rel_err(r, g)
        if not e <= tol:
            return "%s relative error %.3g > %.3g" % (name, e, tol)
    return None


# ---- bit-exact checks of the MFMA kernels on integer data ---------------------------------------
#
# With small-integer operands every product and every f32 partial sum of a convolution / GEMM is an
# exact integer, so the result does not depend on the summation order, the tile shape, the split
# count or atomics: a kernel's output must equal a float64 reference bit for bit, and one wrong
# element fails the comparison (a whole-tensor relative L2 of 1e-2 accepts a pixel that lost a tap,
# and either 1e-2 criterion accepts truncation in place of round-to-nearest-even:
# tests/test_numerics_helper.py).

_F32_EXACT = float(1 << 24)  # integers up to 2^24 are exact in f32 (every partial sum)
_BF16_EXACT = 256.0          # integers up to 2^8 are exact in bf16 (8 significand bits)


def integer_data(shape, kind: str = "sparse", seed: int = 0, device="cpu", hi: int = 4) -> torch.Tensor:
    """A float32 tensor of small integers (cast it to bf16: every value is exact there), drawn on the
    CPU from ``seed`` -- the same values whatever ``device`` it is moved to.

    ``"sparse"``: {-1, 0, 1} with P(non-zero) = 1/4 (the default operand: sums over thousands of
    terms stay within 256); ``"dense"``: {-2, -1, 1, 2}, never zero -- the activation operand next
    to a sparse weight, so a read of the wrong address cannot hide behind a zero; ``"ties"``:
    non-negative integers in [0, hi) -- with {0, 1} weights (``hi=2``) the sums pass 256, where odd
    integers lie exactly halfway between two bf16 values and exercise the rounding mode."""
    g = torch.Generator().manual_seed(seed)
    if kind == "sparse":
        r = torch.randint(0, 8, shape, generator=g)
        t = (r == 0).float() - (r == 1).float()
    elif kind == "dense":
        r = torch.randint(0, 4, shape, generator=g)
        t = torch.tensor([-2.0, -1.0, 1.0, 2.0])[r]
    elif kind == "ties":
        t = torch.randint(0, hi, shape, generator=g).float()
    else:
        raise ValueError(kind)
    return t.to(device)


def tie_fraction(ref_f64: torch.Tensor) -> float:
    """Share of the elements that lie exactly halfway between two adjacent bf16 values (where
    round-to-nearest-even, round-half-away and truncation all differ)."""
    r = ref_f64.double()
    f = r.float()
    assert torch.equal(f.double(), r), "tie_fraction: the reference is not exact in f32"
    low = f.contiguous().view(torch.int32) & 0xFFFF
    return (low == 0x8000).double().mean().item()


def _canon_bits(t: torch.Tensor) -> torch.Tensor:
    """Bit patterns with -0 folded onto +0 (the sign of an exact zero sum depends on the order of
    the additions, in the reference as in the kernel)."""
    t = t.contiguous()
    t = torch.where(t == 0, torch.zeros_like(t), t)
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def check_exact_reference(ref_f64: torch.Tensor, dtype: torch.dtype, ties: bool = False, what: str = "") -> None:
    """The preconditions under which a kernel's ``dtype`` output must equal ``ref_f64`` bit for bit:
    integer-valued, below 2^24 in magnitude (exact in every f32 partial sum) and, for a bf16 output
    outside the ties kind, within 256 (exact in bf16).  Raises AssertionError, never skips."""
    assert ref_f64.dtype == torch.float64, "%s: the reference must be float64" % what
    assert torch.isfinite(ref_f64).all(), "%s: non-finite reference" % what
    assert torch.equal(ref_f64, ref_f64.round()), "%s: the reference is not integer-valued" % what
    mx = ref_f64.abs().max().item() if ref_f64.numel() else 0.0
    assert mx < _F32_EXACT, "%s: reference magnitude %g is not exact in f32 partial sums" % (what, mx)
    if dtype == torch.bfloat16 and not ties:
        assert mx <= _BF16_EXACT, "%s: reference magnitude %g is not exact in bf16" % (what, mx)


def assert_bits_equal(got: torch.Tensor, ref_f64: torch.Tensor, what: str = "", ties: bool = False) -> None:
    """``got`` (bf16 / f32 / f64, any layout) equals ``ref_f64`` rounded to its dtype by torch's own
    f64 -> f32 -> dtype conversion (round-to-nearest-even), bit for bit.  The preconditions are
    enforced on the reference alone (:func:`check_exact_reference`).  A mismatch reports the count,
    the first indices and got / expected at each, so a failure names the pixel and the channel."""
    check_exact_reference(ref_f64, got.dtype, ties, what)
    assert tuple(got.shape) == tuple(ref_f64.shape), "%s: shape %s vs reference %s" % (
        what, tuple(got.shape), tuple(ref_f64.shape))
    exp = ref_f64.to(got.device)
    exp = exp if got.dtype == torch.float64 else exp.float().to(got.dtype)
    g = got.detach().contiguous()  # logical (NCHW) element order: indices read as [n, c, h, w]
    bad = _canon_bits(g) != _canon_bits(exp)
    n = int(bad.sum().item())
    if n == 0:
        return
    idx = bad.nonzero()[:8].cpu()
    lines = ["%s  got %r  expected %r" % (tuple(i.tolist()), g[tuple(i)].item(), exp[tuple(i)].item()) for i in idx]
    raise AssertionError("%s: %d of %d elements differ from the exact reference; first:\n  %s" % (
        what, n, g.numel(), "\n  ".join(lines)))


# ---- element-wise checks of kernels that round a value they know only to within delta -----------
#
# The BN apply kernels compute a handful of f32 operations per element and round once to bf16.
# With general (non-integer) coefficients the f32 value is not exact, but it lies within
# delta = 2^-24 * k * (sum of the magnitudes of the terms) of the f64 value of the same formula
# (k = the f32 roundings on the path).  Rounding is monotone, so the stored value lies between
# RNE(ref - delta) and RNE(ref + delta) -- for almost every element one and the same number.

_SIG_BITS = {torch.bfloat16: 8, torch.float32: 24}
_MIN_EXP = -125  # frexp exponent of the smallest normal f32 / bf16 (2^-126 = 0.5 * 2^-125)


def ulp_of(v_f64: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Spacing of ``dtype`` (bf16 / f32) at each |v|, in float64 (the subnormal spacing below the
    smallest normal number)."""
    _, e = torch.frexp(v_f64.abs())
    e = e.clamp_min(_MIN_EXP).to(torch.float64)
    return torch.exp2(e - _SIG_BITS[dtype])


def round_to(v_f64: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """``v`` rounded to nearest-even in ``dtype`` (bf16 / f32), computed and returned in float64:
    |v| in units of the target ulp (an exact power-of-two scaling), its floor and its fraction.  One
    rounding -- ``v.float().bfloat16()`` rounds twice and merges values closer than an f32 ulp."""
    assert v_f64.dtype == torch.float64
    ulp = ulp_of(v_f64, dtype)
    t = v_f64.abs() / ulp
    fl = torch.floor(t)
    frac = t - fl
    up = (frac > 0.5) | ((frac == 0.5) & (torch.remainder(fl, 2) == 1))
    return torch.copysign((fl + up.to(torch.float64)) * ulp, v_f64)


def rounding_interval(ref_f64: torch.Tensor, delta_f64: torch.Tensor, dtype: torch.dtype, relu: bool = False):
    """(lo, hi, ambiguous): the ``dtype`` values between which a kernel's output must lie when it
    rounds (after a ReLU when ``relu``) an f32 value within ``delta`` of ``ref``; ``ambiguous`` where
    lo != hi, i.e. where [ref - delta, ref + delta] holds a rounding boundary (or, with a ReLU, 0)."""
    a, b = ref_f64 - delta_f64, ref_f64 + delta_f64
    if relu:
        a, b = a.clamp_min(0), b.clamp_min(0)
    lo, hi = round_to(a, dtype), round_to(b, dtype)
    return lo, hi, lo != hi


def assert_rounds_from(got: torch.Tensor, ref_f64: torch.Tensor, delta_f64, what: str = "",
                       max_ambiguous: float = 0.01, relu: bool = False) -> torch.Tensor:
    """``got`` (bf16 / f32) is one rounding away from a value the kernel knows to within ``delta`` of
    ``ref_f64`` (with ``relu``: ``ref_f64`` is the value before a ReLU that precedes the rounding).
    Every element must equal RNE(ref) in ``got.dtype``; only where [ref - delta, ref + delta] straddles
    a rounding boundary may it be either neighbour (with a ReLU and 0 inside the interval: 0 or the
    neighbour).  The share of such ambiguous elements is asserted, on the reference alone, to be at
    most ``max_ambiguous``: a condition on the data recipe, not a measurement of the kernel.  A
    mismatch reports the count, the first indices ([n, c, h, w] for a 4-D tensor) and got / expected.
    Returns the bool tensor of ambiguous elements."""
    assert ref_f64.dtype == torch.float64, "%s: the reference must be float64" % what
    assert got.dtype in _SIG_BITS, "%s: %s output" % (what, got.dtype)
    assert tuple(got.shape) == tuple(ref_f64.shape), "%s: shape %s vs reference %s" % (
        what, tuple(got.shape), tuple(ref_f64.shape))
    ref = ref_f64.to(got.device)
    delta = torch.as_tensor(delta_f64, dtype=torch.float64, device=got.device).expand_as(ref)
    assert torch.isfinite(ref).all() and torch.isfinite(delta).all() and (delta >= 0).all(), \
        "%s: non-finite reference or delta" % what
    lo, hi, amb = rounding_interval(ref, delta, got.dtype, relu)
    share = amb.double().mean().item() if amb.numel() else 0.0
    assert share <= max_ambiguous, "%s: %.3g of the reference elements are ambiguous (cap %.3g): " \
        "the data recipe does not suit this check" % (what, share, max_ambiguous)
    g = got.detach().double()
    bad = ~((g >= lo) & (g <= hi))  # a NaN fails both comparisons
    n = int(bad.sum().item())
    if n:
        exp = round_to(ref.clamp_min(0) if relu else ref, got.dtype)
        idx = bad.nonzero()[:8].cpu()
        lines = []
        for i in idx:
            i = tuple(i.tolist())
            e = "%r" % exp[i].item() if not amb[i].item() else "%r..%r" % (lo[i].item(), hi[i].item())
            lines.append("%s  got %r  expected %s" % (i, g[i].item(), e))
        raise AssertionError("%s: %d of %d elements are not the rounded reference; first:\n  %s" % (
            what, n, g.numel(), "\n  ".join(lines)))
    return amb
