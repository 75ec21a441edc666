"""``ops.conv.wgrad`` lands on the kernel the planner's route names (csrc/kernels/wgrad_plan.cpp
``conv_wgrad_route``): one small shape per route outcome.  The result equals, bit for bit, the binding
called with the route's family and variant (none of these paths uses atomics, so they are reproducible),
or ``aten.convolution_backward`` on the library route, and is within the row-image tests' ``rel < 1e-2``
of an fp32 reference."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = [
    # route, kernel, (N, H, W, Cin, Cout, kh, kw, ph, pw)
    ("square", "Rows3x3", (2, 8, 8, 64, 64, 3, 3, 1, 1)),
    ("square", "Tiled", (2, 8, 8, 64, 128, 1, 1, 0, 0)),
    ("rect", "RowsRing", (4, 25, 25, 48, 64, 5, 5, 2, 2)),
    ("rect", "RowsRect", (3, 12, 12, 128, 128, 1, 7, 0, 3)),
    ("rect", "Tiled", (3, 12, 12, 256, 64, 1, 7, 0, 3)),
    ("library", None, (5, 9, 9, 24, 40, 1, 1, 0, 0)),
]


@pytest.mark.parametrize("route,kernel,shape", CASES, ids=["%s-%s" % (c[0], c[1]) for c in CASES])
def test_wgrad_runs_the_routed_kernel(route, kernel, shape):
    from kungfu_amd._lib import hip
    from kungfu_amd.ops.conv import wgrad

    H = hip()
    N, Hh, W, cin, cout, kh, kw, ph, pw = shape
    got_route, variant, cap = H.conv_wgrad_route(N, Hh, W, cin, cout, kh, kw, ph, pw, 1)
    assert got_route == route
    cl = torch.channels_last
    torch.manual_seed(13)
    x = torch.randn(N, cin, Hh, W, device="cuda").bfloat16().contiguous(memory_format=cl)
    oh, ow = Hh + 2 * ph - kh + 1, W + 2 * pw - kw + 1
    dy = torch.randn(N, cout, oh, ow, device="cuda").bfloat16().contiguous(memory_format=cl)
    w = torch.empty(cout, cin, kh, kw, device="cuda", dtype=torch.bfloat16).contiguous(memory_format=cl)
    dw = wgrad(dy, x, w, 1, (ph, pw))
    if route == "square":
        assert H.conv_wgrad_plan(N, Hh, W, cin, cout, kh, 1, variant)[4] == kernel and N * oh * ow < cap
        want = H.conv_wgrad(dy, x, kh, 1, variant=variant)
    elif route == "rect":
        assert H.conv_wgrad_plan(N, Hh, W, cin, cout, kh, 1, variant, window=(kh, kw, ph, pw))[4] == kernel
        want = H.conv_wgrad_rect(dy, x, kh, kw, 1, ph, pw, variant)
    else:
        want = torch.ops.aten.convolution_backward(dy, x, w, None, [1, 1], [ph, pw], [1, 1], False, [0, 0], 1,
                                                   [False, True, False])[1]
    assert dw.shape == want.shape and dw.dtype == want.dtype and torch.equal(dw, want)
    ref = torch.nn.grad.conv2d_weight(x.float(), (cout, cin, kh, kw), dy.float(), 1, (ph, pw))
    rel = ((dw.float() - ref).norm() / ref.norm()).item()
    assert rel < 1e-2, rel
