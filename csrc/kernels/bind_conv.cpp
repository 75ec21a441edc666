// The MFMA implicit-GEMM family: conv, conv_rect, their data / weight gradients, the weight flips and gemm.
#include "bind_util.hpp"

#include <array>
#include <optional>
#include <vector>

using namespace kfb;

namespace {

const auto kCL = at::MemoryFormat::ChannelsLast;

// General 1x1 / 3x3 convolution with fused epilogues (conv.hip).
// stats: f64 [kStatSlots*2*Cout] zero-initialised workspace receiving sum / sum of squares of the
// bf16 outputs per channel (consumed and re-zeroed by bn_forward(..., sums=stats)).
// out: accumulate target (y = out + conv(x, w), written in place and returned).
// bn_x / bn_fcoef / bn_mask (backward): the output is the gradient of a BN(+ReLU) output whose
// input is bn_x; stats then receive sum(dz), sum(dz * x) (dz = grad * relu') for
// bn_backward(..., sums=stats).  bn_mask (1 bit per element) or bn_fcoef (forward
// [scale; shift]) gives the ReLU gate.
at::Tensor conv(at::Tensor x, at::Tensor w, int64_t stride, OptTensor stats, OptTensor out, int64_t variant,
                OptTensor bn_x, OptTensor bn_fcoef, OptTensor bn_mask, OptTensor bias, bool gate, OptTensor acc_mask,
                bool acc_even) {
    const char *op = "conv";
    check_cl4(x, op, "x", kAnyGpu);
    const Dev dev = x.device();
    check_cl4(w, op, "w", dev);
    TORCH_CHECK(w.size(2) == w.size(3) && w.size(1) == x.size(1), "conv: w must be [Cout, Cin, KS, KS] with x's Cin");
    const auto [N, C, H, W] = dims4(x, op, "x");
    const int K = narrow(w.size(0), op, "w"), ks = narrow(w.size(2), op, "w"), st = narrow(stride, op, "stride");
    TORCH_CHECK(kfk::conv_supported(C, K, ks, st), "conv: unsupported channels/kernel/stride");
    const int pad = (ks - 1) / 2;
    const int OH = (H + 2 * pad - ks) / st + 1, OW = (W + 2 * pad - ks) / st + 1;
    TORCH_CHECK(OH > 0 && OW > 0, "conv: empty output");
    check_extent32(op, "x", {N, H, W, C});
    check_extent32(op, "the output", {N, OH, OW, K});
    const int64_t ysz[4] = {N, K, OH, OW};
    const int64_t ynumel = c10::multiply_integers(at::IntArrayRef(ysz));
    double *sp = stats_ptr(stats, op, K, dev);
    const bool accum = has(out), bwd = has(bn_x);
    kfk::EpiArgs ea;
    ea.stats = sp;
    int epi = accum ? kfk::kEpiAccum : 0;
    if (has(bias)) {
        // relu(conv + bias): VGG's conv + bias + ReLU as the conv epilogue
        TORCH_CHECK(!accum && !sp && !bwd && !gate, "conv: bias epilogue excludes out/stats/bn_x/gate");
        check_dense(*bias, op, "bias", dev, at::kBFloat16, K);
        ea.bias = bf16(*bias);
        epi = kfk::kEpiBiasRelu;
    } else if (gate) {
        // gradient of a ReLU output bn_x: y = conv * (bn_x > 0); stats[slot][0] += sum(y)
        TORCH_CHECK(!accum && sp && bwd && !has(bn_mask) && !has(bn_fcoef),
                    "conv: gate needs stats and bn_x (the ReLU output), no out/bn_mask/bn_fcoef");
        check_cl4(*bn_x, op, "bn_x", dev, ysz);
        ea.bx = bf16(*bn_x);
        epi = kfk::kEpiGate;
    } else if (bwd) {
        epi |= bn_bwd_epilogue(op, ea, ysz, K, dev, sp, bn_x, bn_fcoef, bn_mask);
    } else if (sp) {
        epi |= kfk::kEpiFwdStats;
    }
    TORCH_CHECK(!(epi & kfk::kEpiFwdStats) || !(epi & kfk::kEpiAccum), "conv: stats + accumulate unsupported");
    if (has(acc_mask)) {
        // out = out * acc_mask + conv (out: a raw ReLU-output gradient, acc_mask: that ReLU's bits)
        TORCH_CHECK(accum && !(epi & kfk::kEpiBwdCoef), "conv: acc_mask needs out and excludes bn_fcoef");
        check_dense(*acc_mask, op, "acc_mask", dev, at::kByte, ynumel / 8);
        ea.amask = acc_mask->data_ptr<uint8_t>();
        epi |= kfk::kEpiAccMask;
    }
    if (acc_even) {
        // out holds a stride-2 1x1 data gradient at its even pixels only (conv_dgrad_s2)
        TORCH_CHECK(accum && st == 1 && !(epi & (kfk::kEpiAccMask | kfk::kEpiBwdCoef)),
                    "conv: acc_even needs out, stride 1 and no acc_mask / bn_fcoef");
        epi |= kfk::kEpiAccEven;
    }
    const int var = narrow(variant, op, "variant");
    c10::DeviceGuard gd(x.device());
    auto y = out_or_empty(out, ysz, x.options().memory_format(kCL), op).first;
    kfk::launch_conv(bf16(x), bf16(w), bf16_mut(y), N, H, W, C, K, ks, st, ea, epi, stream_of(x, 0), var);
    return y;
}

// Linear layer on the MFMA kernel: y[M, N] = x[M, K] @ w[N, K]^T (both row-major bf16).
//   bias:            y += bias (bf16 [N]);
//   out:             y = out += x w^T (accumulate into an existing [M, N] bf16 tensor);
//   gelu_u + stats:  y = (x w^T) * gelu'(gelu_u), stats[slot][0][n] += sum_m y (a bias gradient;
//                    stats: zeroed f64 kStatSlots x 2 x N workspace).
std::vector<at::Tensor> gemm(at::Tensor x, at::Tensor w, OptTensor bias, OptTensor out, OptTensor gelu_u,
                             OptTensor stats, int64_t variant) {
    const char *op = "gemm";
    TORCH_CHECK(x.dim() == 2, "gemm: x must be 2-D [M, K]");
    check_dense(x, op, "x", kAnyGpu, at::kBFloat16, x.numel());
    const Dev dev = x.device();
    TORCH_CHECK(w.dim() == 2 && w.size(1) == x.size(1), "gemm: w must be 2-D [N, K] with x's K");
    check_dense(w, op, "w", dev, at::kBFloat16, w.numel());
    const int64_t M = x.size(0), K = x.size(1), N = w.size(0);
    TORCH_CHECK(M < (int64_t(1) << 31) && K < (int64_t(1) << 31) && N < (int64_t(1) << 31) &&
                    kfk::gemm_supported(static_cast<int>(M), static_cast<int>(K), static_cast<int>(N)),
                "gemm: unsupported shape (K, N multiples of 64)");
    kfk::EpiArgs ea;
    int epi = 0;
    auto check_mn = [&](const at::Tensor &t, const char *what) {
        TORCH_CHECK(t.dim() == 2 && t.size(0) == M && t.size(1) == N, "gemm: ", what, " must be 2-D [M, N]");
        check_dense(t, op, what, dev, at::kBFloat16, M * N);
    };
    if (has(out)) {
        TORCH_CHECK(!has(bias) && !has(gelu_u), "gemm: out (accumulate) excludes bias / gelu_u");
        check_mn(*out, "out");
        epi = kfk::kEpiAccum;
    }
    if (has(bias)) {
        check_dense(*bias, op, "bias", dev, at::kBFloat16, N);
        ea.bias = bf16(*bias);
        epi = kfk::kEpiBias;
    }
    if (has(gelu_u)) {
        TORCH_CHECK(epi == 0, "gemm: gelu_u excludes bias / out");
        check_mn(*gelu_u, "gelu_u");
        TORCH_CHECK(has(stats), "gemm: stats must be given with gelu_u (the f64 kStatSlots x 2 x N workspace)");
        ea.bx = bf16(*gelu_u);
        ea.stats = stats_ptr(stats, op, N, dev);
        epi = kfk::kEpiGeluGrad;
    }
    const int var = narrow(variant, op, "variant");
    c10::DeviceGuard gd(x.device());
    auto y = out_or_empty(out, {M, N}, x.options(), op).first;
    kfk::launch_gemm(bf16(x), bf16(w), bf16_mut(y), static_cast<int>(M), static_cast<int>(K), static_cast<int>(N), ea,
                     epi, stream_of(x, 0), var);
    return {y};
}

// Data gradient of a stride-2 1x1 (pad 0) / 3x3 (pad 1) convolution with an even input:
// dy [N, Cout, OH, OW] -> dx [N, Cin, 2OH, 2OW] (channels_last bf16), wt = conv_flip_weight(w)
// [Cin, Cout, ks, ks].  ks = 3: every pixel written (four parity-phase GEMMs); bn_x + stats
// (+ bn_fcoef or bn_mask) also accumulate the backward sums of the BN whose input is bn_x, as
// conv().  ks = 1: only the even pixels are written -- complete dx with a stride-1 data
// gradient conv(..., out=dx, acc_even=True).
at::Tensor conv_dgrad_s2(at::Tensor dy, at::Tensor wt, int64_t ks, OptTensor stats, OptTensor bn_x, OptTensor bn_fcoef,
                         OptTensor bn_mask, int64_t variant, int64_t dh, int64_t dw, int64_t pad) {
    const char *op = "conv_dgrad_s2";
    check_cl4(dy, op, "dy", kAnyGpu);
    const Dev dev = dy.device();
    TORCH_CHECK(ks == 1 || ks == 3, "conv_dgrad_s2: ks must be 1 or 3");
    check_cl4(wt, op, "wt", dev);
    check_cl4(wt, op, "wt", dev, {wt.size(0), dy.size(1), ks, ks});
    const auto [N, K, OH, OW] = dims4(dy, op, "dy");
    const int C = narrow(wt.size(0), op, "wt");
    if (dh <= 0) {
        TORCH_CHECK(kfk::conv_supported(K, C, static_cast<int>(ks), 1), "conv_dgrad_s2: unsupported channels");
        dh = 2 * OH, dw = 2 * OW, pad = ks == 3 ? 1 : 0;
    } else {
        // any dx size (ks = 3, pad 0 | 1): channel counts % 8
        TORCH_CHECK(ks == 3 && (pad == 0 || pad == 1) && K % 8 == 0 && C % 8 == 0 && K >= 16 && C >= 16 && dw > 0 &&
                        (dh + 2 * pad - 3) / 2 + 1 == OH && (dw + 2 * pad - 3) / 2 + 1 == OW,
                    "conv_dgrad_s2: dh/dw/pad do not match a 3x3 stride-2 convolution of dy's size (channels % 8)");
    }
    check_extent32(op, "dx", {N, dh, dw, C});
    const int64_t dxsz[4] = {N, C, dh, dw};
    kfk::EpiArgs ea;
    int epi = 0;
    if (has(bn_x)) {
        TORCH_CHECK(ks == 3, "conv_dgrad_s2: BN sums need every pixel (ks = 3)");
        epi = bn_bwd_epilogue(op, ea, dxsz, C, dev, stats_ptr(stats, op, C, dev), bn_x, bn_fcoef, bn_mask);
    }
    const int var = narrow(variant, op, "variant");
    c10::DeviceGuard gd(dy.device());
    auto dx = at::empty(dxsz, dy.options().memory_format(kCL));
    kfk::launch_conv_dgrad_s2(bf16(dy), bf16(wt), bf16_mut(dx), N, OH, OW, K, C, static_cast<int>(ks), ea, epi,
                              stream_of(dy, 0), var, static_cast<int>(dh), static_cast<int>(dw), static_cast<int>(pad));
    return dx;
}

// The shared tail of the two weight-gradient bindings: dy against the shape, extents, allocate, launch.
at::Tensor wgrad_launch(const char *op, const at::Tensor &dy, const at::Tensor &x, const kfk::WgradPlan &plan,
                        OptTensor out, bool accumulate, bool atomics) {
    const kfk::WgradShape &sh = plan.shape;
    const bool f32 = has(out) && out->scalar_type() == at::kFloat;
    c10::DeviceGuard gd(x.device());
    auto dw = out_or_empty(out, {sh.Cout, sh.Cin, sh.kh, sh.kw},
                           x.options().dtype(f32 ? at::kFloat : at::kBFloat16).memory_format(kCL), op).first;
    at::Tensor ws;
    if (plan.ws_floats > 0) ws = at::empty({plan.ws_floats}, x.options().dtype(at::kFloat));
    kfk::launch_conv_wgrad(bf16(dy), bf16(x), dw.data_ptr(), plan.ws_floats > 0 ? ws.data_ptr<float>() : nullptr, plan,
                           f32, accumulate, stream_of(x, 0), atomics);
    return dw;
}

void wgrad_check(const char *op, const at::Tensor &dy, const at::Tensor &x, const kfk::WgradShape &sh) {
    check_cl4(dy, op, "dy", x.device(), {sh.N, sh.Cout, sh.OH(), sh.OW()});
    check_extent32(op, "x", {sh.N, sh.H, sh.W, sh.Cin});
    check_extent32(op, "dy", {sh.N, sh.OH(), sh.OW(), sh.Cout});
}

// Weight gradient of conv(x, w, stride, pad (ks-1)/2): dw [Cout, Cin, ks, ks] channels_last
// (memory [Cout][ks][ks][Cin]).  out: bf16 or f32 destination of that shape/layout (written,
// or added to with accumulate); otherwise a new bf16 tensor.  variant / splits: -1 = planner.
at::Tensor conv_wgrad(at::Tensor dy, at::Tensor x, int64_t ks, int64_t stride, OptTensor out, bool accumulate,
                      int64_t variant, int64_t splits, bool atomics) {
    const char *op = "conv_wgrad";
    check_cl4(x, op, "x", kAnyGpu);
    check_cl4(dy, op, "dy", Dev(x.device()));
    const auto [N, C, H, W] = dims4(x, op, "x");
    const auto sh = kfk::wgrad_square_shape(N, H, W, C, narrow(dy.size(1), op, "dy"), narrow(ks, op, "ks"),
                                            narrow(stride, op, "stride"));
    TORCH_CHECK(kfk::conv_wgrad_supported(sh.Cin, sh.Cout, sh.kh, sh.stride), "conv_wgrad: unsupported channels/kernel/stride");
    wgrad_check(op, dy, x, sh);
    TORCH_CHECK(has(out) || !accumulate, "conv_wgrad: accumulate needs out");
    const auto plan = kfk::conv_wgrad_plan(sh, kfk::WgradFamily::Square, narrow(variant, op, "variant"),
                                           narrow(splits, op, "splits"));
    return wgrad_launch(op, dy, x, plan, out, accumulate, atomics);
}

// Weight gradient of a KH x KW convolution with zero padding (ph, pw): dw [Cout, Cin, KH, KW]
// channels_last bf16 (kfk::conv_wgrad_rect_supported: Inception-v3's windows / channel counts).
at::Tensor conv_wgrad_rect(at::Tensor dy, at::Tensor x, int64_t kh, int64_t kw, int64_t stride, int64_t ph, int64_t pw,
                           int64_t variant) {
    const char *op = "conv_wgrad_rect";
    check_cl4(x, op, "x", kAnyGpu);
    check_cl4(dy, op, "dy", Dev(x.device()));
    const auto [N, C, H, W] = dims4(x, op, "x");
    const kfk::WgradShape sh{N, H, W, C, narrow(dy.size(1), op, "dy"), narrow(kh, op, "kh"), narrow(kw, op, "kw"),
                             narrow(ph, op, "ph"), narrow(pw, op, "pw"), narrow(stride, op, "stride")};
    TORCH_CHECK(kfk::conv_wgrad_rect_supported(sh.Cin, sh.Cout, sh.kh, sh.kw, sh.stride) && sh.ph >= 0 && sh.pw >= 0 &&
                    sh.ph < sh.kh && sh.pw < sh.kw,
                "conv_wgrad_rect: unsupported channels/window/stride/padding");
    wgrad_check(op, dy, x, sh);
    const auto plan = kfk::conv_wgrad_plan(sh, kfk::WgradFamily::Rect, narrow(variant, op, "variant"));
    return wgrad_launch(op, dy, x, plan, OptTensor(), false, true);
}

// [Cout, Cin, KS, KS] channels_last -> flipped/transposed [Cin, Cout, KS, KS] channels_last
at::Tensor conv_flip_weight(at::Tensor w) {
    const char *op = "conv_flip_weight";
    check_cl4(w, op, "w", kAnyGpu);
    const auto [K, C, kh, kw] = dims4(w, op, "w");
    c10::DeviceGuard gd(w.device());
    auto wt = at::empty({C, K, kh, kw}, w.options().memory_format(kCL));
    kfk::launch_conv_flip_weight_taps(bf16(w), bf16_mut(wt), K, C, kh * kw, stream_of(w, 0));
    return wt;
}

// KH x KW convolution with zero padding (ph, pw) on the MFMA kernel (Inception-v3 shapes,
// kfk::conv_rect_supported); stats: optional f64 [kStatSlots*2*Cout] BN-statistics workspace.
at::Tensor conv_rect(at::Tensor x, at::Tensor w, int64_t stride, int64_t ph, int64_t pw, OptTensor stats, OptTensor out,
                     OptTensor bn_x, OptTensor bn_fcoef) {
    const char *op = "conv_rect";
    check_cl4(x, op, "x", kAnyGpu);
    const Dev dev = x.device();
    check_cl4(w, op, "w", dev);
    TORCH_CHECK(w.size(1) == x.size(1), "conv_rect: w must be [Cout, Cin, KH, KW] with x's Cin");
    const auto [N, C, H, W] = dims4(x, op, "x");
    const auto [K, wc, kh, kw] = dims4(w, op, "w");
    const int st = narrow(stride, op, "stride"), PH = narrow(ph, op, "ph"), PW = narrow(pw, op, "pw");
    TORCH_CHECK(kfk::conv_rect_supported(C, K, kh, kw, st) && PH >= 0 && PW >= 0 && PH < kh && PW < kw,
                "conv_rect: unsupported channels/window/stride/padding");
    const int OH = (H + 2 * PH - kh) / st + 1, OW = (W + 2 * PW - kw) / st + 1;
    TORCH_CHECK(OH > 0 && OW > 0, "conv_rect: empty output");
    check_extent32(op, "x", {N, H, W, C});
    check_extent32(op, "the output", {N, OH, OW, K});
    const int64_t ysz[4] = {N, K, OH, OW};
    kfk::EpiArgs ea;
    ea.stats = stats_ptr(stats, op, K, dev);
    int epi = ea.stats ? kfk::kEpiFwdStats : 0;
    // bn_x: the output is the gradient of a BN+ReLU output whose input is bn_x (forward coefficients
    // bn_fcoef): stats receives that BN's backward sums (sum dz, sum dz*x) instead
    const bool bwd = has(bn_x);
    if (bwd) epi = bn_bwd_epilogue(op, ea, ysz, K, dev, ea.stats, bn_x, bn_fcoef, OptTensor());
    // out: y = out + conv(x, w) in place (e.g. sibling convolutions' data gradients into one dx)
    TORCH_CHECK(!has(out) || epi == 0 || bwd, "conv_rect: out must not be combined with forward stats");
    c10::DeviceGuard gd(x.device());
    auto [y, accum] = out_or_empty(out, ysz, x.options().memory_format(kCL), op);
    if (accum) epi |= kfk::kEpiAccum;
    kfk::launch_conv_rect(bf16(x), bf16(w), bf16_mut(y), N, H, W, C, K, kh, kw, PH, PW, st, ea, epi, stream_of(x, 0));
    return y;
}

// dsts[i] = conv_flip_weight(srcs[i]) for a list of bf16 conv weights, in as few launches as
// possible (FlipTable::kMax per launch).  dsts must be preallocated [Cin, Cout, KS, KS] channels_last.
void conv_flip_weights(std::vector<at::Tensor> srcs, std::vector<at::Tensor> dsts) {
    const char *op = "conv_flip_weights";
    TORCH_CHECK(srcs.size() == dsts.size(), "conv_flip_weights: length mismatch");
    if (srcs.empty()) return;
    c10::DeviceGuard gd(srcs[0].device());
    auto s = stream_of(srcs[0], 0);
    kfk::FlipTable tab;
    tab.start[0] = 0;
    for (size_t i = 0; i < srcs.size(); ++i) {
        const auto &w = srcs[i];
        const auto &d = dsts[i];
        check_cl4(w, op, "srcs", i ? Dev(srcs[0].device()) : kAnyGpu);
        check_cl4(d, op, "dsts", w.device(), {w.size(1), w.size(0), w.size(2), w.size(3)});
        const auto [K, C, kh, kw] = dims4(w, op, "srcs");
        const int k = tab.n;
        tab.src[k] = bf16(w);
        tab.dst[k] = bf16_mut(d);
        tab.cout[k] = K;
        tab.cin[k] = C;
        tab.taps[k] = kh * kw;
        tab.start[k + 1] = tab.start[k] + w.numel();
        tab.n = k + 1;
        if (tab.n == kfk::FlipTable::kMax) {
            kfk::launch_conv_flip_multi(tab, s);
            tab.n = 0;
        }
    }
    kfk::launch_conv_flip_multi(tab, s);
}

}  // namespace

void bind_conv(py::module_ &m) {
    m.def("conv", &conv, "1x1/3x3 NHWC bf16 convolution (MFMA implicit GEMM) with fused BN-statistics and "
          "accumulate epilogues", py::arg("x"), py::arg("w"), py::arg("stride") = 1, py::arg("stats") = py::none(),
          py::arg("out") = py::none(), py::arg("variant") = -1, py::arg("bn_x") = py::none(),
          py::arg("bn_fcoef") = py::none(), py::arg("bn_mask") = py::none(), py::arg("bias") = py::none(),
          py::arg("gate") = false, py::arg("acc_mask") = py::none(), py::arg("acc_even") = false);
    m.def("conv_variants", &kfk::conv_variants);
    m.def("conv_supported", &kfk::conv_supported);
    m.attr("conv_stat_slots") = kfk::kStatSlots;
    m.def("conv_rect", &conv_rect, "KH x KW NHWC bf16 convolution with zero padding (MFMA implicit GEMM; "
          "Inception-v3 windows) with an optional BN-statistics epilogue", py::arg("x"), py::arg("w"),
          py::arg("stride") = 1, py::arg("ph") = 0, py::arg("pw") = 0, py::arg("stats") = py::none(),
          py::arg("out") = py::none(), py::arg("bn_x") = py::none(), py::arg("bn_fcoef") = py::none());
    m.def("conv_rect_supported", &kfk::conv_rect_supported);
    m.def("gemm", &gemm, "linear layer x @ w^T on the MFMA kernel with bias / GELU-gradient(+bias-gradient "
          "sums) / accumulate epilogues", py::arg("x"), py::arg("w"), py::arg("bias") = py::none(),
          py::arg("out") = py::none(), py::arg("gelu_u") = py::none(),
          py::arg("stats") = py::none(), py::arg("variant") = -1);
    m.def("gemm_supported", &kfk::gemm_supported);
    m.def("conv_dgrad_s2", &conv_dgrad_s2, "data gradient of a stride-2 1x1/3x3 NHWC bf16 convolution (parity-phase "
          "MFMA implicit GEMMs)", py::arg("dy"), py::arg("wt"), py::arg("ks"), py::arg("stats") = py::none(),
          py::arg("bn_x") = py::none(), py::arg("bn_fcoef") = py::none(), py::arg("bn_mask") = py::none(),
          py::arg("variant") = -1, py::arg("dh") = 0, py::arg("dw") = 0, py::arg("pad") = 1);
    m.def("conv_wgrad_rect", &conv_wgrad_rect, "weight gradient of a KH x KW padded NHWC bf16 convolution "
          "(split-K MFMA GEMM, any channel count % 8)", py::arg("dy"), py::arg("x"), py::arg("kh"), py::arg("kw"),
          py::arg("stride") = 1, py::arg("ph") = 0, py::arg("pw") = 0, py::arg("variant") = -1);
    m.def("conv_wgrad", &conv_wgrad, "weight gradient of the 1x1/3x3 NHWC bf16 convolution (split-K MFMA GEMM)",
          py::arg("dy"), py::arg("x"), py::arg("ks"), py::arg("stride") = 1, py::arg("out") = py::none(),
          py::arg("accumulate") = false, py::arg("variant") = -1, py::arg("splits") = -1,
          py::arg("atomics") = true);
    // ---- the weight-gradient planner (wgrad_plan.hpp): host-only queries
    m.def("conv_wgrad_supported", &kfk::conv_wgrad_supported);
    m.def("conv_wgrad_rect_supported", &kfk::conv_wgrad_rect_supported);
    m.def("conv_wgrad_variants", [] { return kfk::kWgradSquareVariants; });
    m.def("conv_wgrad_rows_rect_supported", [](int N, int H, int W, int Cin, int Cout, int kh, int kw, int ph, int pw,
                                               int stride) {
        return kfk::conv_wgrad_rows_rect_supported({N, H, W, Cin, Cout, kh, kw, ph, pw, stride});
    }, "a row-image weight-gradient kernel covers this multi-tap window (args: N, H, W, Cin, Cout, kh, kw, ph, pw, stride)");
    m.def("conv_wgrad_rows_rect_auto", [](int N, int H, int W, int Cin, int Cout, int kh, int kw, int ph, int pw,
                                          int stride) {
        return kfk::conv_wgrad_rows_rect_auto({N, H, W, Cin, Cout, kh, kw, ph, pw, stride});
    }, "the row-image variant conv_wgrad_rect(..., WGRAD_ROWS_AUTO) picks for this shape (args: N, H, W, Cin, Cout, kh, "
       "kw, ph, pw, stride)");
    m.def("conv_wgrad_plan", [](int N, int H, int W, int Cin, int Cout, int ks, int stride, int variant, int splits,
                                std::optional<std::array<int, 4>> window) {
        const auto p = window ? kfk::conv_wgrad_plan({N, H, W, Cin, Cout, (*window)[0], (*window)[1], (*window)[2],
                                                      (*window)[3], stride}, kfk::WgradFamily::Rect, variant)
                              : kfk::conv_wgrad_plan(kfk::wgrad_square_shape(N, H, W, Cin, Cout, ks, stride),
                                                     kfk::WgradFamily::Square, variant, splits);
        return py::make_tuple(p.variant, p.splits, p.kps, p.ws_floats, kfk::wgrad_kernel_name(p.kernel));
    }, "(variant, splits, kps, ws_floats, kernel) of conv_wgrad's plan, or with window = (kh, kw, ph, pw) of "
       "conv_wgrad_rect's (ks and splits are then unused)", py::arg("N"), py::arg("H"), py::arg("W"), py::arg("Cin"),
          py::arg("Cout"), py::arg("ks"), py::arg("stride"), py::arg("variant") = -1, py::arg("splits") = -1,
          py::arg("window") = py::none());
    m.def("conv_wgrad_route", [](int N, int H, int W, int Cin, int Cout, int kh, int kw, int ph, int pw, int stride) {
        const auto r = kfk::conv_wgrad_route({N, H, W, Cin, Cout, kh, kw, ph, pw, stride});
        return py::make_tuple(kfk::wgrad_route_name(r.route), r.variant, r.max_pixels);
    }, "(route, variant, max_pixels): 'library', or the family ('square': conv_wgrad, 'rect': conv_wgrad_rect) and the "
       "variant code that take this convolution's weight gradient, and the output pixels one launch handles",
          py::arg("N"), py::arg("H"), py::arg("W"), py::arg("Cin"), py::arg("Cout"), py::arg("kh"), py::arg("kw"),
          py::arg("ph"), py::arg("pw"), py::arg("stride"));
    m.attr("WGRAD_AUTO") = static_cast<int>(kfk::kWgradAuto);
    m.attr("WGRAD_TILE_128x128") = static_cast<int>(kfk::kWgradTile128x128);
    m.attr("WGRAD_TILE_128x64") = static_cast<int>(kfk::kWgradTile128x64);
    m.attr("WGRAD_TILE_64x128") = static_cast<int>(kfk::kWgradTile64x128);
    m.attr("WGRAD_TILE_64x64") = static_cast<int>(kfk::kWgradTile64x64);
    m.attr("WGRAD_TILE_256x128") = static_cast<int>(kfk::kWgradTile256x128);
    m.attr("WGRAD_TILE_128x256") = static_cast<int>(kfk::kWgradTile128x256);
    m.attr("WGRAD_ROWS") = static_cast<int>(kfk::kWgradRows);
    m.attr("WGRAD_TILE_256x256") = static_cast<int>(kfk::kWgradTile256x256);
    m.attr("WGRAD_RING_32x2") = static_cast<int>(kfk::kWgradRing32x2);
    m.attr("WGRAD_RING_32x3") = static_cast<int>(kfk::kWgradRing32x3);
    m.attr("WGRAD_RING_32x4") = static_cast<int>(kfk::kWgradRing32x4);
    m.attr("WGRAD_RING_64x3") = static_cast<int>(kfk::kWgradRing64x3);
    m.attr("WGRAD_RING_64x4") = static_cast<int>(kfk::kWgradRing64x4);
    m.attr("WGRAD_ROWS_AUTO") = static_cast<int>(kfk::kWgradRowsAuto);
    m.def("conv_flip_weight", &conv_flip_weight, "w[co,ci,kh,kw] -> w[ci,co,KS-1-kh,KS-1-kw] (data-gradient weights)");
    m.def("conv_flip_weights", &conv_flip_weights, "multi-tensor conv_flip_weight into preallocated outputs");
}
