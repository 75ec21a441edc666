// Image stems: ResNet's 7x7/2 (stem.hip) and the small 3 -> 32 | 64 windows (stem3.hip).
#include "bind_util.hpp"

using namespace kfb;

namespace {

const auto kCL = at::MemoryFormat::ChannelsLast;

// the [N, 3, H, W] channels_last f32 / bf16 image
void check_img3(const at::Tensor &x, const char *op) {
    TORCH_CHECK(x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kFloat, op,
                ": x must be the [N, 3, H, W] channels_last f32 / bf16 image");
    check_cl4(x, op, "x", kAnyGpu, x.scalar_type());
    TORCH_CHECK(x.size(1) == 3, op, ": x must be the [N, 3, H, W] channels_last f32 / bf16 image");
}

// x [N, 3, H, W] channels_last bf16 -> [N, 4, H, W] channels_last (4th channel zero)
at::Tensor stem_pad4(at::Tensor x) {
    check_img3(x, "stem_pad4");
    c10::DeviceGuard gd(x.device());
    auto x4 = at::empty({x.size(0), 4, x.size(2), x.size(3)}, x.options().dtype(at::kBFloat16).memory_format(kCL));
    const int64_t npix = x.size(0) * x.size(2) * x.size(3);
    if (x.scalar_type() == at::kFloat) kfk::launch_stem_pad4_f32(x.data_ptr<float>(), bf16_mut(x4), npix, stream_of(x, 0));
    else kfk::launch_stem_pad4(bf16(x), bf16_mut(x4), npix, stream_of(x, 0));
    return x4;
}

// w [64, 3, 7, 7] channels_last bf16 -> packed [64, 224] (kh, kw<8, c<4), zero padded
at::Tensor stem_pack_weight(at::Tensor w) {
    check_cl4(w, "stem_pack_weight", "w", kAnyGpu, {64, 3, 7, 7});
    c10::DeviceGuard gd(w.device());
    auto wp = at::empty({64, 224}, w.options());
    kfk::launch_stem_pack_weight(bf16(w), bf16_mut(wp), stream_of(w, 0));
    return wp;
}

// the padded image x4 [N, 4, H, W] of the 7x7 stem: its {N, 4, H, W}
Dims4 stem_x4(const at::Tensor &x4, const char *op) {
    check_cl4(x4, op, "x4", kAnyGpu);
    TORCH_CHECK(x4.size(1) == 4, op, ": x4 must be [N, 4, H, W]");
    return dims4(x4, op, "x4");
}

// y = conv7x7s2p3(x, w) [N, 64, OH, OW] channels_last bf16; stats: BN sums workspace (f64 slots x 2 x 64)
at::Tensor stem_forward(at::Tensor x4, at::Tensor wp, OptTensor stats) {
    const char *op = "stem_forward";
    const auto [N, C4, H, W] = stem_x4(x4, op);
    const Dev dev = x4.device();
    check_dense(wp, op, "wp", dev, at::kBFloat16, 64 * 224);
    TORCH_CHECK(H >= 4 && W >= 4, "stem_forward: input too small");
    double *sp = stats_ptr(stats, op, 64, dev);
    c10::DeviceGuard gd(x4.device());
    auto y = at::empty({N, 64, kfk::stem_out(H), kfk::stem_out(W)}, x4.options().memory_format(kCL));
    kfk::launch_stem_forward(bf16(x4), bf16(wp), bf16_mut(y), sp, N, H, W, stream_of(x4, 0));
    return y;
}

// dw [64, 3, 7, 7] channels_last bf16 from the conv output y, x4 and the pooled gradient dyp / argmax bytes
at::Tensor stem_wgrad_bnp(at::Tensor y, at::Tensor x4, at::Tensor dyp, at::Tensor arg, at::Tensor fcoef,
                          at::Tensor bcoef, int64_t splits) {
    const char *op = "stem_wgrad_bnp";
    const auto [N, C4, H, W] = stem_x4(x4, op);
    const Dev dev = x4.device();
    const int OH = kfk::stem_out(H), OW = kfk::stem_out(W);
    check_cl4(y, op, "y", dev, {N, 64, OH, OW});
    check_cl4(dyp, op, "dyp", dev, {N, 64, kfk::pool_out(OH), kfk::pool_out(OW)});
    check_dense(arg, op, "arg", dev, at::kByte, dyp.numel());
    check_dense(fcoef, op, "fcoef", dev, at::kFloat, 2 * 64);
    check_dense(bcoef, op, "bcoef", dev, at::kFloat, 3 * 64);
    TORCH_CHECK(kfk::stem_wgrad_bnp_supported(N, H, W), "stem_wgrad_bnp: image too wide for the row kernel");
    const int sp = splits > 0 ? narrow(splits, op, "splits") : kfk::stem_wgrad_splits(N, H, W);
    c10::DeviceGuard gd(x4.device());
    auto part = at::empty({kfk::stem_wgrad_workspace(N, H, W, sp)}, x4.options().dtype(at::kFloat));
    auto dw = at::empty({64, 3, 7, 7}, x4.options().memory_format(kCL));
    kfk::launch_stem_wgrad_bnp(bf16(y), bf16(x4), bf16_mut(dw), part.data_ptr<float>(), N, H, W, sp, bf16(dyp),
                               arg.data_ptr<uint8_t>(), fcoef.data_ptr<float>(), bcoef.data_ptr<float>(),
                               stream_of(x4, 0));
    return dw;
}

// dw [64, 3, 7, 7] channels_last bf16 from dy [N, 64, OH, OW] and x4
at::Tensor stem_wgrad(at::Tensor dy, at::Tensor x4, int64_t splits) {
    const char *op = "stem_wgrad";
    const auto [N, C4, H, W] = stem_x4(x4, op);
    check_cl4(dy, op, "dy", x4.device(), {N, 64, kfk::stem_out(H), kfk::stem_out(W)});
    const int sp = splits > 0 ? narrow(splits, op, "splits") : kfk::stem_wgrad_splits(N, H, W);
    c10::DeviceGuard gd(x4.device());
    auto part = at::empty({kfk::stem_wgrad_workspace(N, H, W, sp)}, x4.options().dtype(at::kFloat));
    auto dw = at::empty({64, 3, 7, 7}, x4.options().memory_format(kCL));
    kfk::launch_stem_wgrad(bf16(dy), bf16(x4), bf16_mut(dw), part.data_ptr<float>(), N, H, W, sp, stream_of(x4, 0));
    return dw;
}

// Small image stems (stem3.hip: Inception's Conv2d_1a, VGG-16's first layer): w [32|64, 3, KH, KW] channels_last
// bf16 -> packed [Cout, 64]
at::Tensor stem3_pack_weight(at::Tensor w) {
    const char *op = "stem3_pack_weight";
    check_cl4(w, op, "w", kAnyGpu);
    TORCH_CHECK((w.size(0) == 32 || w.size(0) == 64) && w.size(1) == 3 && w.size(2) <= 4 && w.size(3) <= 4,
                "stem3_pack_weight: w must be [32|64, 3, KH<=4, KW<=4]");
    const auto [Cout, C, kh, kw] = dims4(w, op, "w");
    c10::DeviceGuard gd(w.device());
    auto wp = at::empty({Cout, 64}, w.options().memory_format(at::MemoryFormat::Contiguous));
    kfk::launch_stem3_pack_weight(bf16(w), bf16_mut(wp), Cout, kh, kw, stream_of(w, 0));
    return wp;
}

// the window of a stem3 binding as ints
struct Win {
    int kh, kw, stride, ph, pw;
};
Win stem3_window(const char *op, int64_t kh, int64_t kw, int64_t stride, int64_t ph, int64_t pw) {
    return {narrow(kh, op, "kh"), narrow(kw, op, "kw"), narrow(stride, op, "stride"), narrow(ph, op, "ph"),
            narrow(pw, op, "pw")};
}

// out (optional): the [N, Cout, OH, OW] channels_last bf16 tensor to write (else a new one)
at::Tensor stem3_forward(at::Tensor x, at::Tensor wp, int64_t kh, int64_t kw, int64_t stride, int64_t ph, int64_t pw,
                         OptTensor stats, OptTensor bias, bool relu, OptTensor out) {
    const char *op = "stem3_forward";
    check_img3(x, op);
    const Dev dev = x.device();
    TORCH_CHECK(wp.dim() == 2 && (wp.size(0) == 32 || wp.size(0) == 64) && wp.size(1) == 64,
                "stem3_forward: wp must be the packed [32|64, 64] weights");
    check_dense(wp, op, "wp", dev, at::kBFloat16, wp.numel());
    const int Cout = static_cast<int>(wp.size(0));
    const auto [N, C, H, W] = dims4(x, op, "x");
    const Win k = stem3_window(op, kh, kw, stride, ph, pw);
    double *sp = stats_ptr(stats, op, Cout, dev);
    const float *bp = nullptr;
    if (has(bias)) {
        check_dense(*bias, op, "bias", dev, at::kFloat, Cout);
        bp = bias->data_ptr<float>();
    }
    const int OH = kfk::stem3_out(H, k.kh, k.stride, k.ph), OW = kfk::stem3_out(W, k.kw, k.stride, k.pw);
    TORCH_CHECK(OH > 0 && OW > 0, "stem3_forward: empty output");
    c10::DeviceGuard gd(x.device());
    auto y = out_or_empty(out, {N, Cout, OH, OW}, x.options().dtype(at::kBFloat16).memory_format(kCL), op).first;
    kfk::launch_stem3_forward(x.data_ptr(), x.scalar_type() == at::kFloat, bf16(wp), bf16_mut(y), sp, bp, relu, Cout, N,
                              H, W, k.kh, k.kw, k.stride, k.ph, k.pw, stream_of(x, 0));
    return y;
}

// out (optional): the [Cout, 3, KH, KW] channels_last tensor (f32 if out_f32, else bf16) to write
at::Tensor stem3_wgrad(at::Tensor dy, at::Tensor x, int64_t kh, int64_t kw, int64_t stride, int64_t ph, int64_t pw,
                       bool out_f32, OptTensor out) {
    const char *op = "stem3_wgrad";
    check_img3(x, op);
    const auto [N, C, H, W] = dims4(x, op, "x");
    const Win k = stem3_window(op, kh, kw, stride, ph, pw);
    TORCH_CHECK(k.kh >= 1 && k.kh <= 4 && k.kw >= 1 && k.kw <= 4, "stem3_wgrad: window <= 4x4");
    const int OH = kfk::stem3_out(H, k.kh, k.stride, k.ph), OW = kfk::stem3_out(W, k.kw, k.stride, k.pw);
    TORCH_CHECK(dy.dim() == 4 && (dy.size(1) == 32 || dy.size(1) == 64),
                "stem3_wgrad: dy must be the [N, 32|64, OH, OW] output gradient");
    const int Cout = static_cast<int>(dy.size(1));
    check_cl4(dy, op, "dy", x.device(), {N, Cout, OH, OW});
    c10::DeviceGuard gd(x.device());
    auto dw = out_or_empty(out, {Cout, 3, k.kh, k.kw},
                           x.options().dtype(out_f32 ? at::kFloat : at::kBFloat16).memory_format(kCL), op).first;
    auto part = at::empty({kfk::stem3_wgrad_workspace(Cout, N, H, W, k.kh, k.kw, k.stride, k.ph, k.pw)},
                          x.options().dtype(at::kFloat));
    kfk::launch_stem3_wgrad(bf16(dy), x.data_ptr(), x.scalar_type() == at::kFloat, dw.data_ptr(), out_f32,
                            part.data_ptr<float>(), Cout, N, H, W, k.kh, k.kw, k.stride, k.ph, k.pw, stream_of(x, 0));
    return dw;
}

}  // namespace

void bind_stem(py::module_ &m) {
    m.def("stem_pad4", &stem_pad4, "[N,3,H,W] bf16/f32 -> [N,4,H,W] channels_last bf16 (zero 4th channel)");
    m.def("stem_pack_weight", &stem_pack_weight, "[64,3,7,7] stem weights -> packed [64,224] for stem_forward");
    m.def("stem_forward", &stem_forward, "7x7/2 pad-3 stem conv on MFMA with fused BN statistics",
          py::arg("x4"), py::arg("wp"), py::arg("stats") = py::none());
    m.def("stem_wgrad", &stem_wgrad, "stem conv weight gradient (split-K MFMA)", py::arg("dy"), py::arg("x4"),
          py::arg("splits") = -1);
    m.def("stem_wgrad_bnp", &stem_wgrad_bnp, "stem conv weight gradient with dy formed from the BN+ReLU+MaxPool "
          "backward while staging (the BN input gradient is never materialised)", py::arg("y"), py::arg("x4"),
          py::arg("dyp"), py::arg("arg"), py::arg("fcoef"), py::arg("bcoef"), py::arg("splits") = -1);
    m.def("stem_wgrad_bnp_supported", &kfk::stem_wgrad_bnp_supported);
    m.def("stem3_pack_weight", &stem3_pack_weight, "pack [32|64, 3, KH, KW] stem weights for stem3_forward");
    m.def("stem3_forward", &stem3_forward, "small image-stem conv (<= 4x4 window, 3 -> 32 | 64 channels) with optional "
          "f32 bias (+ ReLU) and BN-sums epilogues", py::arg("x"), py::arg("wp"), py::arg("kh"), py::arg("kw"),
          py::arg("stride"), py::arg("ph"), py::arg("pw"), py::arg("stats") = py::none(), py::arg("bias") = py::none(),
          py::arg("relu") = false, py::arg("out") = py::none());
    m.def("stem3_wgrad", &stem3_wgrad, "its weight gradient (MFMA over pixels, deterministic)", py::arg("dy"),
          py::arg("x"), py::arg("kh"), py::arg("kw"), py::arg("stride"), py::arg("ph"), py::arg("pw"),
          py::arg("out_f32") = false, py::arg("out") = py::none());
}
