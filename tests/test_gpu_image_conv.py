"""The 64-channel image stem (csrc/kernels/stem3.hip at Cout 64: VGG-16's 3 -> 64 first layer) on the GPU.

Bit-exact forward (plain + BN statistics, bias, bias + ReLU, round-to-nearest-even through the bias epilogue),
bit-exact deterministic weight gradient, the grid-stride loops past the grid caps, guard rows, the bindings'
refusals, the autograd op against f32 torch, and the VGG-16 routing (fused stack and layered path) with its
model-level accuracy against an f32 run.  The integer-data recipes and their float64 references come from
tests/test_image_conv_cases.py, which checks every precondition on the CPU."""
import pytest
import torch
import torch.nn.functional as F

import test_image_conv_cases as C
from kungfu_amd.utils.numerics import assert_bits_equal, rel_err

pytestmark = pytest.mark.gpu

CO = C.COUT


@pytest.fixture(scope="module")
def H():
    from kungfu_amd._lib import hip

    return hip()


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _dev(t):
    """A CPU integer tensor as the kernels take it: bf16 on the GPU, channels_last when 4-D."""
    t = t.cuda().bfloat16()
    return _cl(t) if t.dim() == 4 else t.contiguous()


def _images(x):
    """The bf16 and the f32 channels_last image of a CPU integer tensor."""
    return _dev(x), _cl(x.cuda())


def _stats(H):
    return torch.zeros(H.conv_stat_slots * 2 * CO, dtype=torch.float64, device="cuda")


# ---- 1. exact forward ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,h,w,k,s,p", C.CASES)
def test_forward_exact(H, n, h, w, k, s, p):
    c = C.fwd_case(n, h, w, k, s, p)
    wp = H.stem3_pack_weight(_dev(c["w"]))
    assert wp.shape == (CO, 64)
    bias = c["bias"].cuda()
    for img in _images(c["x"]):
        what = "stem3_forward Cout 64 %dx%d k%d s%d from %s: " % (h, w, k, s, img.dtype)
        st = _stats(H)
        y = H.stem3_forward(img, wp, k, k, s, p, p, st)
        assert y.is_contiguous(memory_format=torch.channels_last)
        assert_bits_equal(y, c["ref"], what + "plain [n, co, oh, ow]")
        sums = st.view(-1, 2, CO).sum(0)
        assert_bits_equal(sums[0], c["s1"], what + "sum y")
        assert_bits_equal(sums[1], c["s2"], what + "sum y^2")
        assert_bits_equal(H.stem3_forward(img, wp, k, k, s, p, p, None, bias), c["with_bias"], what + "bias")
        assert_bits_equal(H.stem3_forward(img, wp, k, k, s, p, p, bias=bias, relu=True), c["bias_relu"],
                          what + "bias + relu")
        # both epilogues: the statistics are of the stored (clamped) bf16 values
        st = _stats(H)
        y = H.stem3_forward(img, wp, k, k, s, p, p, st, bias, True)
        assert_bits_equal(y, c["bias_relu"], what + "bias + relu + stats")
        sums = st.view(-1, 2, CO).sum(0)
        assert_bits_equal(sums[0], c["bias_relu"].sum((0, 2, 3)), what + "sum relu(y + bias)")
        assert_bits_equal(sums[1], (c["bias_relu"] ** 2).sum((0, 2, 3)), what + "sum relu(y + bias)^2")


# ---- 2. rounding mode through the bias epilogue --------------------------------------------------------------

def test_forward_bias_epilogue_rounds_ties_to_even(H):
    (n, h, w, k, s, p), _ = C.TIES
    c = C.ties_case()
    wp = H.stem3_pack_weight(_dev(c["w"]))
    bias = c["bias"].cuda()
    for img in _images(c["x"]):
        y = H.stem3_forward(img, wp, k, k, s, p, p, None, bias, True)
        assert_bits_equal(y, c["bias_relu"], "stem3_forward ties bias + relu from %s" % img.dtype, ties=True)


# ---- 3. exact weight gradient --------------------------------------------------------------------------------

@pytest.mark.parametrize("n,h,w,k,s,p", C.CASES)
def test_wgrad_exact(H, n, h, w, k, s, p):
    g = C.wgrad_case(n, h, w, k, s, p)
    dy = _dev(g["dy"])
    for img in _images(g["x"]):
        what = "stem3_wgrad Cout 64 %dx%d k%d s%d from %s " % (h, w, k, s, img.dtype)
        d32 = H.stem3_wgrad(dy, img, k, k, s, p, p, out_f32=True)
        assert d32.shape == (CO, 3, k, k) and d32.is_contiguous(memory_format=torch.channels_last)
        assert_bits_equal(d32, g["ref"], what + "f32 [co, c, kh, kw]")
        d16 = H.stem3_wgrad(dy, img, k, k, s, p, p)
        assert_bits_equal(d16, g["ref"], what + "bf16 [co, c, kh, kw]")
        assert torch.equal(d32, H.stem3_wgrad(dy, img, k, k, s, p, p, out_f32=True))
        assert torch.equal(d16, H.stem3_wgrad(dy, img, k, k, s, p, p))


# ---- 4. the grid-stride loops --------------------------------------------------------------------------------

def test_forward_grid_stride_loop(H):
    n, h, w, k, s, p = C.BIG_FWD
    c = C.big_fwd_case()
    wp = H.stem3_pack_weight(_dev(c["w"]))
    y = H.stem3_forward(_cl(c["x"].cuda()), wp, k, k, s, p, p, None, c["bias"].cuda(), True)
    assert_bits_equal(y, c["bias_relu"], "stem3_forward past the grid cap, bias + relu")


def test_wgrad_grid_stride_loop(H):
    n, h, w, k, s, p = C.BIG_WGRAD
    g = C.big_wgrad_case()
    dw = H.stem3_wgrad(_dev(g["dy"]), _cl(g["x"].cuda()), k, k, s, p, p, out_f32=True)
    assert_bits_equal(dw, g["ref"], "stem3_wgrad past the grid cap, f32")


# ---- 5. guard rows -------------------------------------------------------------------------------------------

_GUARD = 512  # rows past M: more than the tallest tile


def _guarded(shape, dtype):
    """A poisoned channels_last buffer of shape[0] + guard leading entries, its leading view and a copy of
    the sentinel entries behind it."""
    per = 1
    for d in shape[2:]:
        per *= d
    extra = (_GUARD + per - 1) // per
    big = _cl(torch.full((shape[0] + extra,) + tuple(shape[1:]), -776.0, dtype=dtype, device="cuda"))
    return big, big[:shape[0]], big[shape[0]:].clone()


@pytest.mark.parametrize("n,h,w,k,s,p", [C.CASES[0], C.CASES[3]])
def test_guard_rows(H, n, h, w, k, s, p):
    c = C.fwd_case(n, h, w, k, s, p)
    wp = H.stem3_pack_weight(_dev(c["w"]))
    big, out, guard = _guarded(c["ref"].shape, torch.bfloat16)
    assert out.is_contiguous(memory_format=torch.channels_last)
    y = H.stem3_forward(_dev(c["x"]), wp, k, k, s, p, p, None, c["bias"].cuda(), True, out=out)
    assert y.data_ptr() == out.data_ptr()
    assert_bits_equal(out, c["bias_relu"], "guarded stem3_forward")
    assert torch.equal(big[n:], guard), "stem3_forward stored past M"
    g = C.wgrad_case(n, h, w, k, s, p)
    for f32 in (True, False):
        big, out, guard = _guarded(g["ref"].shape, torch.float32 if f32 else torch.bfloat16)
        H.stem3_wgrad(_dev(g["dy"]), _dev(g["x"]), k, k, s, p, p, out_f32=f32, out=out)
        assert_bits_equal(out, g["ref"], "guarded stem3_wgrad f32 %s" % f32)
        assert torch.equal(big[CO:], guard), "stem3_wgrad stored past channel 63"


# ---- 6. binding refusals -------------------------------------------------------------------------------------

def test_binding_refusals(H):
    n, h, w, k, s, p = C.CASES[0]
    c = C.fwd_case(n, h, w, k, s, p)
    x = _dev(c["x"])
    wp = H.stem3_pack_weight(_dev(c["w"]))
    bias = c["bias"].cuda()
    err = (RuntimeError, ValueError)
    with pytest.raises(err, match="stem3_pack_weight"):
        H.stem3_pack_weight(_dev(torch.zeros(48, 3, k, k)))
    with pytest.raises(err, match="wp must be"):
        H.stem3_forward(x, torch.zeros(48, 64, dtype=torch.bfloat16, device="cuda"), k, k, s, p, p)
    with pytest.raises(err, match="wp must be"):
        H.stem3_forward(x, wp.view(-1), k, k, s, p, p)
    with pytest.raises(err, match="bias must be"):
        H.stem3_forward(x, wp, k, k, s, p, p, None, c["bias"])  # a CPU bias
    with pytest.raises(err, match="bias must be"):
        H.stem3_forward(x, wp, k, k, s, p, p, None, bias.bfloat16())
    with pytest.raises(err, match="bias must be"):
        H.stem3_forward(x, wp, k, k, s, p, p, None, bias[:32].contiguous())
    with pytest.raises(err, match="bias must be"):
        H.stem3_forward(x, wp, k, k, s, p, p, None, torch.zeros(2 * CO, device="cuda")[::2])  # strided
    with pytest.raises(err, match="stats must be"):
        H.stem3_forward(x, wp, k, k, s, p, p, torch.zeros(H.conv_stat_slots * 2 * 32, dtype=torch.float64, device="cuda"))
    oh, ow = C.out_hw(h, w, k, s, p)
    for ch in (48, 16):
        with pytest.raises(err, match="dy must be"):
            H.stem3_wgrad(torch.zeros(n, ch, oh, ow, dtype=torch.bfloat16, device="cuda").contiguous(
                memory_format=torch.channels_last), x, k, k, s, p, p)
    dy32 = _cl(torch.zeros(n, 32, oh, ow, dtype=torch.bfloat16, device="cuda"))
    with pytest.raises(err, match="out must be"):  # a 32-channel dy cannot fill a 64-channel gradient
        H.stem3_wgrad(dy32, x, k, k, s, p, p, out=_cl(torch.zeros(CO, 3, k, k, dtype=torch.bfloat16, device="cuda")))
    # the existing positional forms still run
    st = _stats(H)
    assert_bits_equal(H.stem3_forward(x, wp, k, k, s, p, p, st), c["ref"], "positional stem3_forward")


# ---- 7. autograd op ------------------------------------------------------------------------------------------

def test_stem3_conv_bias_relu_autograd_matches_fp32():
    """stem3_conv(..., bias, relu=True) under bf16 autocast from an f32 image, f32 weight and f32 bias, against the
    f32 torch relu(conv2d + b) chain of the same operands: relative L2 below 1e-2 (output) and 2e-2 (dw, db), and
    the figures of tests/test_gpu.py::test_stem3_forward_and_wgrad_match_fp32 (output max error within
    2^-7 max|ref| + 1e-3; gradients 1e-5).

    As in that test the image and the weight hold bf16-representable values, so the reference multiplies what
    the kernel multiplies.  With unrounded operands the gradients say nothing about the kernel: rounding x and w
    to bf16 moves an output near zero across the ReLU gate (about 3 of a channel's 4292 pixels here), and db,
    a sum of +-1-sized terms whose norm is only ~sqrt(pixels / 2), then differs by 3.6 % (dw 4.0 %) from the f32
    chain although every product is exact (measured; the output differs by 0.28 %, the rounding itself)."""
    from kungfu_amd.ops.stem import stem3_conv, stem3_eligible

    torch.manual_seed(71)
    conv = torch.nn.Conv2d(3, CO, 3, padding=1).cuda()
    with torch.no_grad():
        conv.weight.copy_((conv.weight * 3.0).bfloat16().float())
        conv.bias.copy_(torch.randn(CO, device="cuda") * 0.3)
    x = _cl(torch.randn(4, 3, 37, 29, device="cuda").bfloat16().float())
    gy = torch.randn(4, CO, 37, 29, device="cuda").bfloat16()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert stem3_eligible(conv, x)
        y = stem3_conv(conv, x, conv.weight, bias=conv.bias, relu=True)
    assert y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=torch.channels_last)
    y.backward(gy)
    dw, db = conv.weight.grad, conv.bias.grad
    assert dw.dtype == torch.float32 and db.dtype == torch.float32 and x.grad is None
    rw = conv.weight.detach().clone().requires_grad_(True)
    rb = conv.bias.detach().clone().requires_grad_(True)
    ry = torch.relu(F.conv2d(x, rw, rb, padding=1))
    ry.backward(gy.float())
    ry = ry.detach()
    err = (y.float() - ry).abs().max().item()
    figs = {"y": rel_err(ry, y.float()), "y max": err, "dw": rel_err(rw.grad, dw), "db": rel_err(rb.grad, db)}
    print("stem3_conv vs f32:", figs)
    assert figs["y"] < 1e-2 and figs["dw"] < 2e-2 and figs["db"] < 2e-2, figs
    assert max(figs["y"], figs["dw"], figs["db"]) < 0.5
    assert err <= 2 ** -7 * ry.abs().max().item() + 1e-3, figs
    assert figs["dw"] < 1e-5 and figs["db"] < 1e-5, figs


# ---- 8. routing, 9. model level ------------------------------------------------------------------------------

class _Spies:
    def __init__(self, monkeypatch, H):
        self.fwd = self.wgrad = self.conv2d_3 = self.convbwd_3 = 0
        of, ow, oc, ob = H.stem3_forward, H.stem3_wgrad, F.conv2d, torch.ops.aten.convolution_backward

        def fwd(*a, **k):
            self.fwd += 1
            return of(*a, **k)

        def wgrad(*a, **k):
            self.wgrad += 1
            return ow(*a, **k)

        def conv2d(x, *a, **k):
            self.conv2d_3 += int(x.shape[1] == 3)
            return oc(x, *a, **k)

        def convbwd(dy, x, *a, **k):
            self.convbwd_3 += int(x.shape[1] == 3)
            return ob(dy, x, *a, **k)

        monkeypatch.setattr(H, "stem3_forward", fwd)
        monkeypatch.setattr(H, "stem3_wgrad", wgrad)
        monkeypatch.setattr(F, "conv2d", conv2d)
        monkeypatch.setattr(torch.ops.aten, "convolution_backward", convbwd)

    def take(self):
        out = (self.fwd, self.wgrad, self.conv2d_3, self.convbwd_3)
        self.fwd = self.wgrad = self.conv2d_3 = self.convbwd_3 = 0
        return out


def _vgg_step(m, x, tgt, fused, amp=True):
    from kungfu_amd.ops.vgg_fused import FusedVGGFeatures

    m.zero_grad(set_to_none=True)
    orig = FusedVGGFeatures.forward
    if not fused:
        FusedVGGFeatures.forward = torch.nn.Sequential.forward
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            out = m(x)
            loss = F.cross_entropy(out.float(), tgt)
        loss.backward()
    finally:
        FusedVGGFeatures.forward = orig
    return out.float().detach(), {k: p.grad.detach().float().clone() for k, p in m.named_parameters()}


def test_vgg16_first_layer_runs_on_stem3(H, monkeypatch):
    """VGG-16's 3 -> 64 first layer goes through stem3_forward / stem3_wgrad exactly once per step, on the fused
    stack and on the layered path, and no library convolution sees the 3-channel image; with the stem switch off
    the library path runs and stem3 is not called."""
    from kungfu_amd.models.vgg import vgg16
    from kungfu_amd.ops import stem as stem_ops

    torch.manual_seed(35)
    m = vgg16(fused_bn=True).cuda().to(memory_format=torch.channels_last).eval()
    x = _cl(torch.randn(2, 3, 64, 64, device="cuda"))
    tgt = torch.randint(0, 1000, (2,), device="cuda")
    spies = _Spies(monkeypatch, H)
    for fused in (True, False):
        _, g = _vgg_step(m, x, tgt, fused)
        assert spies.take() == (1, 1, 0, 0), "fused %s" % fused
        assert all(torch.isfinite(v).all() for v in g.values())
        assert g["features.0.weight"].abs().sum() > 0 and g["features.0.bias"].abs().sum() > 0
    old = stem_ops.set_enabled(False)
    try:
        for fused in (True, False):
            _vgg_step(m, x, tgt, fused)
            f, w, c3, b3 = spies.take()
            assert (f, w) == (0, 0) and c3 == 1, "stem off, fused %s" % fused
    finally:
        stem_ops.set_enabled(old)


def test_vgg16_with_stem3_first_layer_is_as_close_to_f32_as_the_library_path():
    """The criterion of tests/test_gpu.py::test_vgg16_fused_stack_matches_layered: against an f32 run of the same
    weights, the fused stack and the layered path with the first layer on stem3 are as close as the layered path
    with the stem switch off (the library first layer)."""
    from kungfu_amd.models.vgg import vgg16
    from kungfu_amd.ops import stem as stem_ops

    torch.manual_seed(33)
    m = vgg16(fused_bn=True).cuda().to(memory_format=torch.channels_last).eval()  # no dropout masks
    x = _cl(torch.randn(4, 3, 64, 64, device="cuda"))
    tgt = torch.randint(0, 1000, (4,), device="cuda")
    new = {"fused": _vgg_step(m, x, tgt, True), "layered": _vgg_step(m, x, tgt, False)}
    old = stem_ops.set_enabled(False)
    try:
        o0, g0 = _vgg_step(m, x, tgt, False)
    finally:
        stem_ops.set_enabled(old)
    of, gf = _vgg_step(m, x, tgt, False, amp=False)
    rel = lambda a, b: ((a - b).norm() / (b.norm() + 1e-12)).item()  # noqa: E731
    for name, (o1, g1) in new.items():
        assert rel(o1, of) < 1.5 * rel(o0, of) + 1e-3, name
        for k in gf:
            e1, e0 = rel(g1[k], gf[k]), rel(g0[k], gf[k])
            assert e1 < 1.5 * e0 + 0.02, (name, k, e1, e0)
