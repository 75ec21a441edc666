"""Inputs, weights and references for the conv epilogue's f32 -> bf16 rounding and for its pixel
addressing (tests/test_rounding_cases.py on the CPU, tests/test_gpu_conv_rounding.py on the GPU).

Rounding recipe.  The input has 64 channels; channels 2j and 2j + 1 of a pixel hold a pair (a, b) of
bf16 values, and output channel co has exactly two weights equal to one, at input channels 2j and 2j + 1
with j = co % 32 (for a 3x3 window both at the centre tap), all others zero.  Every accumulator is then
(+0 + a) + b: products with a zero weight are (signed) zeros, and a + b is exact in f32 by construction,
so the f32 value the epilogue rounds is known exactly, whatever the order of the sum.  The reference is
that f32 value rounded by torch on the CPU (`.bfloat16()`).  No input is an infinity or a NaN (0 * inf
would poison every channel of the pixel); `nan_input` builds the NaN case on pixels of its own.

Slot (pixel m, pair j) takes class (32 m + j) % len(CLASSES); the classes, by the f32 sum v:
  tie_even_below / tie_even_above   the low 16 bits of v are exactly 0x8000, bit 16 clear / set
  near_tie_below / near_tie_above   the nearest sums either side of a tie that two bf16 terms can form:
                                    low 16 bits 0x7f80 and 0x8100.  (A sum ONE f32 ulp from a tie, low
                                    bits 0x7fff / 0x8001, cannot be made from two bf16 values: in units
                                    of the f32 ulp the sum is odd, so one term is an odd integer below
                                    256, the other a multiple of 2^16, and their sum is +-(1..255) mod
                                    2^16, never 0x8001 or 0x7fff.  The bias epilogue adds a third
                                    term: one_ulp_input / one_ulp_bias build those sums there, and
                                    the CPU test checks the two patterns on the integer formula.)
  exact                             low 16 bits zero: bf16 values already
  binade_up                         rounding carries into the next binade (255.5 ulp -> 256 ulp)
  overflow                          finite bf16 terms whose sum rounds to +-inf (finite in f32: max bf16
                                    plus half its ulp; and infinite in f32 already: max + max)
  subnormal                         sums of bf16 subnormals: f32-subnormal values, exact in bf16
  zero_pos / zero_neg               (+0, +0) and (-0, -0) inputs.  The accumulator starts at +0, so both
                                    give +0: a conv output is never -0 (a - a = +0 too)
each with both signs of (a, b) where a sign applies.

Addressing recipe.  x[pixel p, channel c] = (7 p + 3 c) % 120 + 1 on the even channels and (5 p + c) % 127 + 1
on the odd ones, small integers whose pair sums (at most 247) are exact in bf16.  Every output adds one even and
one odd channel, so the two co-prime periods make a decode that is off by fewer than 15,240 pixels show (no tile,
image or persistent m-tile stride of the cases is a multiple of that).  Output channel co reads (tap ta, channel ca) and (tap tb, channel cb) that differ from
channel to channel, so a wrong row, tap or image decode shows as a wrong element."""
import numpy as np
import torch

CIN = 64
CLASSES = ["tie_even_below", "tie_even_above", "near_tie_below", "near_tie_above", "exact", "binade_up",
           "overflow", "subnormal", "zero"]
SIGNED = [(c, s) for c in CLASSES for s in (0, 1)]  # (class, sign bit)
MIN_PER_CLASS = 64


def _bf16_bits(sign, biased_exp, mant):
    return (sign << 15) | (biased_exp << 7) | mant


def _pair(cls, sign, rng, finite=False):
    """One (a, b) pair of bf16 bit patterns of class `cls`, both with sign bit `sign`.
    a = A * 2^E with the 8-bit significand A in [128, 255]: biased exponent E + 134, mantissa A - 128.
    finite: exponents within 2^+-20 and no overflow class (it becomes `exact`), for the epilogues that sum the
    outputs and their squares in f32."""
    E = int(rng.integers(-20, 20)) if finite else int(rng.integers(-90, 90))
    if finite and cls == "overflow":
        cls = "exact"
    A = int(rng.integers(128, 254))
    if cls == "tie_even_below":
        A &= ~1
        b = _bf16_bits(sign, E - 1 + 127, 0)  # 2^(E-1): half a bf16 ulp of a
    elif cls == "tie_even_above":
        A |= 1
        b = _bf16_bits(sign, E - 1 + 127, 0)
    elif cls == "near_tie_below":
        b = _bf16_bits(sign, E + 125, 127)  # 255 * 2^(E-9) = 2^(E-1) (1 - 1/256)
    elif cls == "near_tie_above":
        b = _bf16_bits(sign, E + 126, 1)  # 129 * 2^(E-8) = 2^(E-1) (1 + 1/128)
    elif cls == "exact":
        A = int(rng.integers(128, 200))
        k, m = int(rng.integers(0, 5)), int(rng.integers(0, 2))  # b = (1 or 1.5) * 2^(k + 1) * 2^E <= 48 * 2^E
        b = _bf16_bits(sign, E + k + 1 + 127, 0x40 * m) if rng.integers(0, 8) else 0
    elif cls == "binade_up":
        A = 255
        b = _bf16_bits(sign, E - 1 + 127, 0x40 * int(rng.integers(0, 2)))  # 0.5 or 0.75 ulp
    elif cls == "overflow":
        A, E = 255, 120  # the largest finite bf16, 0x7f7f
        b = _bf16_bits(sign, E - 1 + 127, 0) if rng.integers(0, 2) else _bf16_bits(sign, E + 134, 127)
    elif cls == "subnormal":
        a = _bf16_bits(sign, 0, int(rng.integers(1, 64)))  # a + b < 128 units of 2^-133: still subnormal
        return a, _bf16_bits(sign, 0, int(rng.integers(0, 64)))
    elif cls == "zero":
        return _bf16_bits(sign, 0, 0), _bf16_bits(sign, 0, 0)
    else:
        raise ValueError(cls)
    return _bf16_bits(sign, E + 134, A - 128), b


def from_bits(bits):
    """uint16 bit patterns (numpy) -> a torch.bfloat16 CPU tensor of the same shape."""
    return torch.from_numpy(np.ascontiguousarray(bits).astype(np.uint16).view(np.int16)).view(torch.bfloat16)


def to_bits(t):
    """A bf16 tensor (any device) -> its bit patterns as an int32 CPU tensor."""
    return t.detach().cpu().contiguous().view(torch.int16).to(torch.int32) & 0xffff


def rounding_input(N, H, W, seed=0, finite=False):
    """x [N, 64, H, W] bf16 (channels_last memory, CPU) of the rounding recipe (finite: see _pair)."""
    rng = np.random.default_rng(1000 + seed)
    M = N * H * W
    bits = np.zeros((M, CIN), dtype=np.uint16)
    for m in range(M):
        for j in range(CIN // 2):
            cls, sign = SIGNED[(32 * m + j) % len(SIGNED)]
            bits[m, 2 * j], bits[m, 2 * j + 1] = _pair(cls, sign, rng, finite)
    return from_bits(bits).view(N, H, W, CIN).permute(0, 3, 1, 2)


def _position_rows(M, C):
    p = torch.arange(M, dtype=torch.int64).view(-1, 1)
    c = torch.arange(C, dtype=torch.int64).view(1, -1)
    v = torch.where(c % 2 == 0, (7 * p + 3 * c) % 120 + 1, (5 * p + c) % 127 + 1)
    return v.to(torch.float32).bfloat16()


def position_input(N, H, W, C=CIN):
    """The position-encoding input (module docstring) as [N, C, H, W] bf16 (channels_last memory, CPU)."""
    return _position_rows(N * H * W, C).view(N, H, W, C).permute(0, 3, 1, 2)


def nan_input(N, H, W):
    """The addressing input with a NaN (quiet and signalling patterns, both signs) in one channel of every
    fifth pixel."""
    rows = _position_rows(N * H * W, CIN)
    pats = from_bits(np.array([0x7fc0, 0xffc0, 0x7f81, 0xffff, 0x7fff], dtype=np.uint16))
    for i, m in enumerate(range(0, rows.shape[0], 5)):
        rows[m, (3 * i) % CIN] = pats[i % len(pats)]
    return rows.view(N, H, W, CIN).permute(0, 3, 1, 2)


def taps_of(co, ks, centre):
    """The two (tap, input channel) positions of output channel co that hold a one."""
    j = co % (CIN // 2)
    if centre or ks == 1:
        t = (ks * ks) // 2
        return (t, 2 * j), (t, 2 * j + 1)
    return (co % (ks * ks), 2 * j), ((2 * co + 1) % (ks * ks), 2 * j + 1)


def weights(Cout, ks, centre=True, Cin=CIN):
    """w [Cout, Cin, ks, ks] bf16 (channels_last memory, CPU), two ones per output channel."""
    w = torch.zeros(Cout, ks * ks, Cin)
    for co in range(Cout):
        for t, ci in taps_of(co, ks, centre):
            w[co, t, ci] = 1.0
    return w.view(Cout, ks, ks, Cin).permute(0, 3, 1, 2).bfloat16()


def conv_sum(x, Cout, ks, stride=1, centre=True):
    """The exact f32 accumulators (+0 + a) + b of conv(x, weights(Cout, ks, centre)), pad (ks - 1) / 2, as
    [N, Cout, OH, OW] float32 (CPU): a gather, no multiplication and no other summand."""
    N, C, H, W = x.shape
    pad = (ks - 1) // 2
    xf = torch.nn.functional.pad(x.float(), (pad, pad, pad, pad))
    OH, OW = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    out = torch.zeros(N, Cout, OH, OW)
    for co in range(Cout):
        (ta, ca), (tb, cb) = taps_of(co, ks, centre)
        va = xf[:, ca, ta // ks:ta // ks + stride * OH:stride, ta % ks:ta % ks + stride * OW:stride]
        vb = xf[:, cb, tb // ks:tb // ks + stride * OH:stride, tb % ks:tb % ks + stride * OW:stride]
        out[:, co] = (0.0 + va) + vb
    return out


def round_int(v):
    """The kernels' integer round-to-nearest-even (common.hpp f32_to_bf16) on a float32 tensor -> bf16 bits."""
    u = v.contiguous().view(torch.int32).to(torch.int64) & 0xffffffff
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffffffff
    return (u >> 16).to(torch.int32)


def classify(v):
    """Class name -> boolean mask over the float32 tensor v, from v's own bits (independent of how the inputs
    were built).  `_neg` / `_pos` suffixes by the sign bit."""
    u = v.contiguous().view(torch.int32).to(torch.int64) & 0xffffffff
    sign, expo, low, bit16 = u >> 31, (u >> 23) & 0xff, u & 0xffff, (u >> 16) & 1
    r = round_int(v).to(torch.int64)
    rexp = (r >> 7) & 0xff
    normal = (expo > 0) & (expo < 255)
    masks = {
        "tie_even_below": normal & (low == 0x8000) & (bit16 == 0),
        "tie_even_above": normal & (low == 0x8000) & (bit16 == 1) & (rexp == expo),
        "near_tie_below": normal & (low >= 0x7f00) & (low < 0x8000),
        "near_tie_above": normal & (low > 0x8000) & (low <= 0x8100) & (rexp == expo),
        "exact": normal & (low == 0),
        "binade_up": normal & (rexp == expo + 1) & (rexp < 255),
        "overflow": (rexp == 255) & ((r & 0x7f) == 0),
        "subnormal": (expo == 0) & ((u & 0x7fffffff) != 0),
        "zero": (u & 0x7fffffff) == 0,
    }
    out = {}
    for k, m in masks.items():
        out[k + "_pos"] = m & (sign == 0)
        out[k + "_neg"] = m & (sign == 1)
    return out


def one_ulp_input(N, H, W):
    """The bias epilogue adds a third term, so there a sum ONE f32 ulp from a tie exists: pair j of every pixel
    is (A * 2^E, 2^(E-1)) with E = j - 16 fixed per pair (an exact tie, A of both parities over the pixels), and
    one_ulp_bias adds +-2^(E-16), one f32 ulp of the sum (24 significant bits: exact in f32).  Positive values
    only: the epilogue's ReLU clears the rest."""
    M = N * H * W
    bits = np.zeros((M, CIN), dtype=np.uint16)
    for m in range(M):
        for j in range(CIN // 2):
            E, A = j - 16, 128 + (7 * m + 3 * j) % 127
            bits[m, 2 * j], bits[m, 2 * j + 1] = _bf16_bits(0, E + 134, A - 128), _bf16_bits(0, E - 1 + 127, 0)
    return from_bits(bits).view(N, H, W, CIN).permute(0, 3, 1, 2)


def one_ulp_bias(cout):
    """bias[co] = +2^(E-16) for the first occurrence of pair j = co % 32, -2^(E-16) for the next, alternating."""
    bits = [_bf16_bits((co // 32) & 1, (co % 32) - 16 - 16 + 127, 0) for co in range(cout)]
    return from_bits(np.array(bits, dtype=np.uint16))
