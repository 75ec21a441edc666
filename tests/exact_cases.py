"""Inputs and float64 references of the bit-exact integer-data tests (tests/test_gpu_exact.py).

Everything here runs on the CPU and never imports the HIP extension: tests/test_numerics_helper.py
walks the same tables through the same builders and asserts every magnitude / tie-share
precondition, so a precondition can never fail first on the GPU machine.  Tensors are float32 / float64
NCHW on the CPU holding small integers (kungfu_amd.utils.numerics.integer_data); the GPU tests cast
them to bf16 channels_last.  Each builder returns a dict whose ``"refs"`` entry lists
``(name, ref_f64, dtype, ties)`` for every exact comparison made from it and whose ``"sums"`` entry lists
``(name, rows, max_abs_term)`` for every per-channel f32 partial sum that must stay exact."""
import functools
import zlib

import torch
import torch.nn.functional as F

from kungfu_amd.utils.numerics import integer_data, unpack_mask

BF16 = torch.bfloat16
F32 = torch.float32


def seed_of(*key) -> int:
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


# ---- shape tables (N, H, W, Cin, Cout): H != W so a row / column swap shows -----------------------
CONV = {"A": (3, 9, 11, 64, 256),    # M = 297: a 256-row tile + 41 rows (224: + 73); one K-step per tap
        "B": (2, 7, 5, 192, 256),    # M = 70 < one tile; three K-steps per tap
        "C": (5, 14, 14, 128, 64)}   # M = 980; Cout = 64: the 256x64 tile only
AB_VARIANTS = (-1, 0, 1, 2, 7, 8)
C_VARIANTS = (-1, 2)
V11 = [("A", 1), ("A", 3), ("C", 1), ("C", 3)]  # conv(..., variant=11): 256x32 tiles, 8 / 2 of them across Cout
# (case, ks, stride)
FWD = [(c, ks, s) for c in ("A", "B") for ks in (1, 3) for s in (1, 2)] + [("C", 1, 1), ("C", 3, 1)]
# ties: (case, ks, hi) -- x in [0, hi), w in {0, 1}; on the default variant and on 7 and 8
FWD_TIES = [("A", 3, 4), ("A", 1, 16)]
TIES_VARIANTS = (-1, 7, 8)
# row-image stride-1 3x3 variants (variant, N, H, W, Cin, Cout): the smallest shapes each accepts with an
# image boundary inside a tile and a tile ending past M (20: 512-row tiles, two of them)
ROWS = [(20, 3, 13, 15, 64, 64), (21, 3, 9, 11, 192, 128), (22, 3, 9, 11, 128, 256), (23, 3, 9, 11, 64, 128),
        (24, 3, 9, 11, 64, 64), (25, 3, 9, 11, 64, 128)]
# epilogues: (ks, variant, shape)
EPI = [(ks, v, CONV["A"]) for ks in (1, 3) for v in (-1, 7, 8)] + [(3, 21, (3, 9, 11, 192, 128))]

# stride-2 data gradient (N, OH, OW) and channel pairs (Cout, Cin)
S2_GRID = (3, 5, 6)
S2_EVEN_PAIRS = [(128, 64), (64, 192), (64, 128)]  # Cin 128: the 128x128 / 256x128 phase tiles
S2_ANY = [(11, 13, 0), (9, 11, 1)]  # dh, dw, pad
S2_ANY_PAIRS = [(128, 64), (64, 192), (96, 72)]

RECT_WINDOWS = [(1, 7, 0, 3), (7, 1, 3, 0), (1, 3, 0, 1), (3, 1, 1, 0), (5, 5, 2, 2), (3, 3, 0, 0)]  # kh, kw, ph, pw
RECT_IMAGE = (2, 9, 11)
RECT_CIN = 128
RECT_COUT = (192, 128, 32)  # 256x64, 256x128 and the 256x32 tile (variant 11 of the conv kernel)

# weight gradients (N, Cin, H, W, Cout)
WGRAD = [(3, 64, 9, 11, 256), (2, 192, 7, 5, 64),
         (2, 256, 7, 5, 256)]  # the two shapes above admit the 128x64 and 64x64 tiles only; this one admits every tile
WGRAD_TIES = ((3, 64, 9, 11, 256), 1, 1, 5)  # shape, ks, stride, hi
WGRAD_RECT_CH = (48, 96)
WGRAD_RECT_IMAGE = (2, 9, 11)

GEMM = [(297, 64, 256), (70, 192, 256), (520, 256, 192)]
GEMM_NT_MN = (257, 768)
GEMM_NT_K = (32, 96, 192)  # one 32-wide slab; three slabs, not a multiple of 64; 192
GEMM_NT_BN = (-1, 128, 192, 256, 1128, 1256)
GEMM_NT_TIES = (192, 6)  # K, hi
GEMM_NT_LD = [(17, 64, 9), (300, 256, 1000)]

STEM_IMAGES = [(3, 37, 45), (1, 16, 9)]
STEM3 = [(4, 20, 18, 2, 1, 0), (2, 29, 31, 3, 1, 1)]  # n, h, w, k, stride, pad


def _operands(xshape, wshape, kind, hi, key):
    if kind == "ties":
        return (integer_data(xshape, "ties", seed_of("x", key), hi=hi),
                integer_data(wshape, "ties", seed_of("w", key), hi=2))
    first = "dense" if kind == "dense_x" else kind  # "dense_x": a dense image with a sparse gradient (the stems)
    return integer_data(xshape, first, seed_of("x", key)), integer_data(wshape, "sparse", seed_of("w", key))


@functools.lru_cache(maxsize=None)
def conv_case(N, H, W, Cin, Cout, kh, kw, stride, ph, pw, kind="dense", hi=4):
    """y = conv(x, w): x ``kind`` ("dense" / "sparse" / "ties"), w sparse ({0, 1} for ties)."""
    key = ("conv", N, H, W, Cin, Cout, kh, kw, stride, ph, pw, kind, hi)
    x, w = _operands((N, Cin, H, W), (Cout, Cin, kh, kw), kind, hi, key)
    ref = F.conv2d(x.double(), w.double(), stride=stride, padding=(ph, pw))
    return {"x": x, "w": w, "ref": ref, "refs": [("y", ref, BF16, kind == "ties")], "sums": []}


def _bits(mask, like):
    """1-bit mask bytes -> a 0/1 float64 tensor shaped like the NCHW tensor ``like``."""
    N, C, H, W = like.shape
    return unpack_mask(mask, N * H * W, C).double().view(N, H, W, C).permute(0, 3, 1, 2)


def dyadic_coef(C, key):
    """Forward BN [scale; shift] with scale in {0.5, 1, 2} and shift in {-1.5, -0.5, 0.5}: on integer x the
    gate argument x * scale + shift is exact in f32 (and in one FMA), so its sign is decided alike
    everywhere (an exact zero, e.g. 1 * 0.5 - 0.5, is off on both sides)."""
    g = torch.Generator().manual_seed(seed_of("coef", key))
    sc = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=g)]
    sh = torch.tensor([-1.5, -0.5, 0.5])[torch.randint(0, 3, (C,), generator=g)]
    return torch.cat([sc, sh])


def bn_sums(grad, bx, on):
    """(dz, sum dz, sum dz * x) per channel of dz = grad * on in float64 (NCHW inputs)."""
    dz = grad * on
    return dz, dz.sum((0, 2, 3)), (dz * bx.double()).sum((0, 2, 3))


@functools.lru_cache(maxsize=None)
def epilogue_case(N, H, W, Cin, Cout, ks):
    """The fused epilogues of ``conv`` on a stride-1 dense-x / sparse-w convolution."""
    base = conv_case(N, H, W, Cin, Cout, ks, ks, 1, (ks - 1) // 2, (ks - 1) // 2)
    key = ("epi", N, H, W, Cin, Cout, ks)
    y = base["ref"]
    M = N * y.shape[2] * y.shape[3]
    g = torch.Generator().manual_seed(seed_of("mask", key))
    c = dict(base)
    c["old"] = integer_data(y.shape, "sparse", seed_of("old", key)) * 3
    c["bias"] = integer_data((Cout,), "dense", seed_of("bias", key)) * 4
    c["relu_out"] = integer_data(y.shape, "dense", seed_of("gate", key)).clamp_min(0)  # a ReLU output: {0, 1, 2}
    c["bx"] = integer_data(y.shape, "dense", seed_of("bx", key))
    c["amask"] = torch.randint(0, 256, (y.numel() // 8,), dtype=torch.uint8, generator=g)
    c["bmask"] = torch.randint(0, 256, (y.numel() // 8,), dtype=torch.uint8, generator=g)
    c["fcoef"] = dyadic_coef(Cout, key)
    c["s1"], c["s2"] = y.sum((0, 2, 3)), (y * y).sum((0, 2, 3))
    c["acc"] = y + c["old"].double()
    c["bias_relu"] = (y + c["bias"].double().view(1, -1, 1, 1)).clamp_min(0)
    c["gated"] = y * (c["relu_out"] > 0)
    c["gated_s1"] = c["gated"].sum((0, 2, 3))
    c["acc_mask"] = c["old"].double() * _bits(c["amask"], y) + y
    _, c["am_s1"], c["am_s2"] = bn_sums(c["acc_mask"], c["bx"], _bits(c["bmask"], y))
    sc, sh = c["fcoef"][:Cout].double().view(1, -1, 1, 1), c["fcoef"][Cout:].double().view(1, -1, 1, 1)
    on = (c["bx"].double() * sc + sh > 0).double()
    _, c["co_s1"], c["co_s2"] = bn_sums(y, c["bx"], on)
    _, c["mk_s1"], c["mk_s2"] = bn_sums(y, c["bx"], _bits(c["bmask"], y))
    c["refs"] = [("y", y, BF16, False), ("acc", c["acc"], BF16, False), ("bias_relu", c["bias_relu"], BF16, False),
                 ("gated", c["gated"], BF16, False), ("acc_mask", c["acc_mask"], BF16, False)]
    ymax, amax = y.abs().max().item(), c["acc_mask"].abs().max().item()
    c["sums"] = [("sum y", M, ymax), ("sum y^2", M, ymax * ymax), ("sum dz*x (coef)", M, 2 * ymax),
                 ("sum dz*x (mask)", M, 2 * amax)]
    return c


@functools.lru_cache(maxsize=None)
def dgrad_case(N, OH, OW, Cout, Cin, ks, stride, pad, dh, dw, kind="dense"):
    """dx [N, Cin, dh, dw] = the data gradient of conv(., w [Cout, Cin, ks, ks], stride, pad) at dy."""
    key = ("dgrad", N, OH, OW, Cout, Cin, ks, stride, pad, dh, dw, kind)
    dy, w = _operands((N, Cout, OH, OW), (Cout, Cin, ks, ks), kind, 4, key)
    ref = torch.nn.grad.conv2d_input((N, Cin, dh, dw), w.double(), dy.double(), stride=stride, padding=pad)
    c = {"dy": dy, "w": w, "ref": ref, "refs": [("dx", ref, BF16, False)], "sums": []}
    if ks == 3 and stride == 2:
        c["bx"] = integer_data(ref.shape, "dense", seed_of("bx", key))
        c["fcoef"] = dyadic_coef(Cin, key)
        sc, sh = c["fcoef"][:Cin].double().view(1, -1, 1, 1), c["fcoef"][Cin:].double().view(1, -1, 1, 1)
        _, c["co_s1"], c["co_s2"] = bn_sums(ref, c["bx"], (c["bx"].double() * sc + sh > 0).double())
        c["sums"] = [("sum dz*x", N * dh * dw, 2 * ref.abs().max().item())]
    return c


@functools.lru_cache(maxsize=None)
def dgrad_pair_case(N, OH, OW, Cout, Cin):
    """The ResNet downsample pair: a stride-2 1x1 data gradient (even pixels of dx) completed by a stride-1
    1x1 data gradient accumulated at the even pixels and stored at the others."""
    a = dgrad_case(N, OH, OW, Cout, Cin, 1, 2, 0, 2 * OH, 2 * OW)
    b = dgrad_case(N, 2 * OH, 2 * OW, Cout, Cin, 1, 1, 0, 2 * OH, 2 * OW, "sparse")
    ref = a["ref"] + b["ref"]
    return {"dy2": a["dy"], "w2": a["w"], "dy1": b["dy"], "w1": b["w"], "ref": ref, "even": a["ref"],
            "refs": [("dx", ref, BF16, False), ("dx even", a["ref"], BF16, False)], "sums": []}


@functools.lru_cache(maxsize=None)
def wgrad_case(N, Cin, H, W, Cout, kh, kw, stride, ph, pw, kind="sparse", hi=4):
    """dw [Cout, Cin, kh, kw]: every operand sparse, so the bf16 result stays within 256 (ties: x in [0, hi),
    dy in {0, 1})."""
    key = ("wgrad", N, Cin, H, W, Cout, kh, kw, stride, ph, pw, kind, hi)
    OH, OW = (H + 2 * ph - kh) // stride + 1, (W + 2 * pw - kw) // stride + 1
    x, dy = _operands((N, Cin, H, W), (N, Cout, OH, OW), kind, hi, key)
    ref = torch.nn.grad.conv2d_weight(x.double(), (Cout, Cin, kh, kw), dy.double(), stride=stride, padding=(ph, pw))
    base = integer_data(ref.shape, "sparse", seed_of("base", key)) * 5
    acc = ref + base.double()
    ties = kind == "ties"
    return {"x": x, "dy": dy, "ref": ref, "base": base, "acc": acc, "sums": [],
            "refs": [("dw", ref, BF16, ties), ("dw f32", ref, F32, ties)] +
                    ([] if ties else [("dw + base", acc, BF16, False), ("dw + base f32", acc, F32, False)])}


@functools.lru_cache(maxsize=None)
def gemm_case(M, K, N, kind="dense", hi=4):
    """c = a [M, K] . b [N, K]^T with an integer bias and an integer accumulate target."""
    key = ("gemm", M, K, N, kind, hi)
    a, b = _operands((M, K), (N, K), kind, hi, key)
    ref = a.double() @ b.double().t()
    ties = kind == "ties"
    c = {"a": a, "b": b, "ref": ref, "refs": [("c", ref, BF16, ties)], "sums": []}
    if not ties:
        c["bias"] = integer_data((N,), "dense", seed_of("bias", key)) * 4
        c["old"] = integer_data((M, N), "sparse", seed_of("old", key)) * 3
        c["with_bias"] = ref + c["bias"].double()
        c["acc"] = ref + c["old"].double()
        c["acc_bias"] = c["with_bias"] + c["old"].double()
        c["refs"] += [("c + bias", c["with_bias"], BF16, False), ("c + old", c["acc"], BF16, False),
                      ("c + bias + old", c["acc_bias"], BF16, False)]
    return c


def stat_sums(case, rows):
    """Adds the forward-statistics references (sum y, sum y^2 per channel) of ``case["ref"]``."""
    y = case["ref"]
    c = dict(case)
    c["s1"], c["s2"] = y.sum((0, 2, 3)), (y * y).sum((0, 2, 3))
    ymax = y.abs().max().item()
    c["sums"] = list(case["sums"]) + [("sum y", rows, ymax), ("sum y^2", rows, ymax * ymax)]
    return c


def all_cases():
    """(label, case) for every data recipe the GPU tests use."""
    for name, ks, s in FWD:
        N, H, W, Ci, Co = CONV[name]
        yield "fwd %s ks%d s%d" % (name, ks, s), conv_case(N, H, W, Ci, Co, ks, ks, s, (ks - 1) // 2, (ks - 1) // 2)
    for name, ks, hi in FWD_TIES:
        N, H, W, Ci, Co = CONV[name]
        yield "fwd ties %s ks%d" % (name, ks), conv_case(N, H, W, Ci, Co, ks, ks, 1, (ks - 1) // 2, (ks - 1) // 2,
                                                         "ties", hi)
    for v, N, H, W, Ci, Co in ROWS:
        yield "rows %d" % v, stat_sums(conv_case(N, H, W, Ci, Co, 3, 3, 1, 1, 1), N * H * W)
    for ks, v, (N, H, W, Ci, Co) in EPI:
        yield "epilogues ks%d v%d" % (ks, v), epilogue_case(N, H, W, Ci, Co, ks)
    N, OH, OW = S2_GRID
    for Co, Ci in S2_EVEN_PAIRS:
        yield "dgrad s2 even %d->%d" % (Co, Ci), dgrad_case(N, OH, OW, Co, Ci, 3, 2, 1, 2 * OH, 2 * OW)
        yield "dgrad s2 1x1 pair %d->%d" % (Co, Ci), dgrad_pair_case(N, OH, OW, Co, Ci)
    for dh, dw, pad in S2_ANY:
        for Co, Ci in S2_ANY_PAIRS:
            yield "dgrad s2 %dx%d p%d %d->%d" % (dh, dw, pad, Co, Ci), dgrad_case(N, OH, OW, Co, Ci, 3, 2, pad, dh, dw)
    for name in ("A", "B"):
        N, H, W, Ci, Co = CONV[name]
        for ks in (1, 3):
            yield "dgrad s1 %s ks%d" % (name, ks), dgrad_case(N, H, W, Co, Ci, ks, 1, (ks - 1) // 2, H, W)
    N, H, W = RECT_IMAGE
    for kh, kw, ph, pw in RECT_WINDOWS:
        for Co in RECT_COUT:
            for s in (1, 2):
                OH, OW = (H + 2 * ph - kh) // s + 1, (W + 2 * pw - kw) // s + 1
                yield "rect %dx%d s%d ->%d" % (kh, kw, s, Co), stat_sums(
                    conv_case(N, H, W, RECT_CIN, Co, kh, kw, s, ph, pw), N * OH * OW)
    for N, Ci, H, W, Co in WGRAD:
        for ks in (1, 3):
            for s in (1, 2):
                yield "wgrad ks%d s%d %d->%d" % (ks, s, Ci, Co), wgrad_case(N, Ci, H, W, Co, ks, ks, s, (ks - 1) // 2,
                                                                         (ks - 1) // 2)
    (N, Ci, H, W, Co), ks, s, hi = WGRAD_TIES
    yield "wgrad ties", wgrad_case(N, Ci, H, W, Co, ks, ks, s, 0, 0, "ties", hi)
    N, H, W = WGRAD_RECT_IMAGE
    for kh, kw, ph, pw in RECT_WINDOWS:
        for s in (1, 2):
            Ci, Co = WGRAD_RECT_CH
            yield "wgrad rect %dx%d s%d" % (kh, kw, s), wgrad_case(N, Ci, H, W, Co, kh, kw, s, ph, pw)
    for M, K, Nn in GEMM:
        yield "gemm %dx%dx%d" % (M, K, Nn), gemm_case(M, K, Nn)
    for K in GEMM_NT_K:
        yield "gemm_nt K%d" % K, gemm_case(GEMM_NT_MN[0], K, GEMM_NT_MN[1])
    yield "gemm_nt ties", gemm_case(GEMM_NT_MN[0], GEMM_NT_TIES[0], GEMM_NT_MN[1], "ties", GEMM_NT_TIES[1])
    for M, K, Nn in GEMM_NT_LD:
        yield "gemm_nt_ld %dx%dx%d" % (M, K, Nn), gemm_case(M, K, Nn)
    for N, H, W in STEM_IMAGES:
        OH, OW = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
        yield "stem fwd %dx%d" % (H, W), stat_sums(conv_case(N, H, W, 3, 64, 7, 7, 2, 3, 3), N * OH * OW)
        yield "stem wgrad %dx%d" % (H, W), wgrad_case(N, 3, H, W, 64, 7, 7, 2, 3, 3, "dense_x")
    for n, h, w, k, s, p in STEM3:
        OH, OW = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        yield "stem3 fwd %dx%d" % (h, w), stat_sums(conv_case(n, h, w, 3, 32, k, k, s, p, p), n * OH * OW)
        yield "stem3 wgrad %dx%d" % (h, w), wgrad_case(n, 3, h, w, 32, k, k, s, p, p, "dense_x")
