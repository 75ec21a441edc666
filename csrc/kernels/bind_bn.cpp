// Fused NHWC BatchNorm (+residual, +ReLU, +MaxPool) forward / backward.
#include "bind_util.hpp"

#include <string>
#include <vector>

using namespace kfb;

namespace {

const auto kCL = at::MemoryFormat::ChannelsLast;

kfk::BNShape bn_shape(const at::Tensor &x, const char *op) {
    check_cl4(x, op, "x", kAnyGpu);
    const int C = narrow(x.size(1), op, "x");
    TORCH_CHECK(kfk::bn_supported_channels(C), op, ": unsupported channel count ", C);
    return kfk::BNShape{x.numel() / C, C};
}

// The checked parameters of one BN as the forward descriptor: everything but the outputs, sums and partial.
kfk::BnFinDesc bn_common(const char *op, kfk::BNShape sh, const Dev &dev, const at::Tensor &weight,
                         const at::Tensor &bias, const OptTensor &running_mean, const OptTensor &running_var,
                         const OptTensor &num_batches, bool training, double momentum, double eps) {
    check_dense(weight, op, "weight", dev, at::kFloat, sh.channels);
    check_dense(bias, op, "bias", dev, at::kFloat, sh.channels);
    kfk::BnFinDesc d;
    d.rows = sh.rows, d.C = sh.channels;
    d.gamma = weight.data_ptr<float>(), d.beta = bias.data_ptr<float>();
    d.momentum = static_cast<float>(momentum), d.eps = static_cast<float>(eps);
    if (has(running_mean)) {
        TORCH_CHECK(has(running_var), op, ": running_var missing");
        d.run_mean = running_mean->data_ptr<float>();
        d.run_var = running_var->data_ptr<float>();
    }
    TORCH_CHECK(training || d.run_mean, op, ": eval mode needs running stats");
    if (training && has(num_batches)) {
        TORCH_CHECK(num_batches->scalar_type() == at::kLong && num_batches->numel() == 1 && num_batches->is_cuda(),
                    op, ": num_batches_tracked must be a 1-element int64 GPU tensor");
        d.nbt = num_batches->data_ptr<int64_t>();
    }
    return d;
}

// {mean, invstd, coef}: the forward's f32 outputs ([C], [C], [scale; shift] = [2C]); out_stats points d at them.
std::vector<at::Tensor> alloc_stats(int C, const at::TensorOptions &fopt) {
    return {at::empty({C}, fopt), at::empty({C}, fopt), at::empty({2 * C}, fopt)};
}

void out_stats(kfk::BnFinDesc &d, const std::vector<at::Tensor> &st) {
    d.mean = st[0].data_ptr<float>(), d.invstd = st[1].data_ptr<float>(), d.coef = st[2].data_ptr<float>();
}

// The scratch of a statistics / reduce pass.
at::Tensor alloc_partial(kfk::BNShape sh, const at::TensorOptions &fopt) {
    return at::empty({2 * static_cast<int64_t>(kfk::bn_num_chunks(sh)) * sh.channels}, fopt);
}

// What a backward takes from its forward: mean / invstd / weight [C] and fcoef [2C], checked, as the
// backward descriptor without its outputs.  `s`: "s" where the arguments are lists of them.
kfk::BnBwdFinDesc bn_saved(const char *op, kfk::BNShape sh, const Dev &dev, const at::Tensor &mean,
                           const at::Tensor &invstd, const at::Tensor &weight, const at::Tensor &fcoef,
                           const char *s = "") {
    const int C = sh.channels;
    const auto name = [s](const char *n) { return std::string(n) + s; };
    check_dense(mean, op, name("mean").c_str(), dev, at::kFloat, C);
    check_dense(invstd, op, name("invstd").c_str(), dev, at::kFloat, C);
    check_dense(weight, op, name("weight").c_str(), dev, at::kFloat, C);
    check_dense(fcoef, op, name("fcoef").c_str(), dev, at::kFloat, 2 * C);
    kfk::BnBwdFinDesc d;
    d.rows = sh.rows, d.C = C;
    d.gamma = weight.data_ptr<float>(), d.mean = mean.data_ptr<float>(), d.invstd = invstd.data_ptr<float>();
    return d;
}

// {dweight, dbias, coef}: the backward's f32 outputs ([C], [C], [k1; k2; k3] = [3C]), d pointed at them.
std::vector<at::Tensor> alloc_bwd_out(kfk::BnBwdFinDesc &d, const at::TensorOptions &fopt) {
    std::vector<at::Tensor> o{at::empty({d.C}, fopt), at::empty({d.C}, fopt), at::empty({3 * d.C}, fopt)};
    d.dgamma = o[0].data_ptr<float>(), d.dbeta = o[1].data_ptr<float>(), d.coef = o[2].data_ptr<float>();
    return o;
}

// The output gradient of a BN: x's shape, bf16, on its device.  Read in place when it is channels_last or a
// 16-byte aligned channel slice of a wider channels_last tensor (a concatenation's gradient; *ld = its row
// stride), else through a channels_last copy.  Call after every other check: the copy is a launch.
at::Tensor bn_dy(at::Tensor dy, const at::Tensor &x, int C, int64_t *ld) {
    *ld = 0;
    if (dy.is_contiguous(kCL)) return dy;
    const int64_t s3 = dy.stride(3);
    const bool slice = dy.stride(1) == 1 && s3 >= C && s3 % 8 == 0 && dy.stride(2) == dy.size(3) * s3 &&
                       dy.stride(0) == dy.size(2) * dy.size(3) * s3 &&
                       reinterpret_cast<uintptr_t>(dy.data_ptr()) % 16 == 0;
    if (!slice) return dy.contiguous(kCL);
    *ld = s3;
    return dy;
}

void check_bn_dy(const at::Tensor &dy, const at::Tensor &x, const char *op) {
    TORCH_CHECK(dy.scalar_type() == at::kBFloat16 && dy.sizes() == x.sizes() && dy.device() == x.device(), op,
                ": dy must be a bf16 tensor of x's shape on its device");
}

// Batched sums-finalize of several training-mode BNs (each with its producing conv's f64 slotted
// sums): ONE launch; returns [mean, invstd, coef] per BN for bn_forward(..., pre=...).
std::vector<std::vector<at::Tensor>> bn_finalize_multi(std::vector<at::Tensor> xs, std::vector<at::Tensor> sums,
                                                       std::vector<at::Tensor> weights, std::vector<at::Tensor> biases,
                                                       std::vector<OptTensor> running_means,
                                                       std::vector<OptTensor> running_vars,
                                                       std::vector<OptTensor> num_batches,
                                                       std::vector<double> momentum, std::vector<double> eps) {
    const char *op = "bn_finalize_multi";
    const size_t n = xs.size();
    TORCH_CHECK(n >= 1 && n <= static_cast<size_t>(kfk::kBnFinMax) && sums.size() == n && weights.size() == n &&
                    biases.size() == n && running_means.size() == n && running_vars.size() == n &&
                    num_batches.size() == n && momentum.size() == n && eps.size() == n,
                "bn_finalize_multi: 1..8 BNs, every list of the same length");
    kfk::BnFinBatch b{};
    b.n = static_cast<int>(n);
    const Dev dev = xs[0].device();
    for (size_t i = 0; i < n; ++i) {
        auto sh = bn_shape(xs[i], op);
        TORCH_CHECK(xs[i].device() == *dev, "bn_finalize_multi: xs must be on one device");
        b.d[i] = bn_common(op, sh, dev, weights[i], biases[i], running_means[i], running_vars[i], num_batches[i], true,
                           momentum[i], eps[i]);
        TORCH_CHECK(sums[i].defined(), "bn_finalize_multi: sums must be defined");
        b.d[i].sums = stats_ptr(sums[i], op, sh.channels, dev, "sums");
    }
    std::vector<std::vector<at::Tensor>> out;
    for (size_t i = 0; i < n; ++i) {
        out.push_back(alloc_stats(b.d[i].C, xs[i].options().dtype(at::kFloat)));
        out_stats(b.d[i], out.back());
    }
    c10::DeviceGuard gd(xs[0].device());
    kfk::launch_bn_sums_finalize_multi(b, stream_of(xs[0], 0));
    return out;
}

// Returns (y, mean, invstd, coef, mask-or-undefined).
std::vector<at::Tensor> bn_forward(at::Tensor x, OptTensor res, at::Tensor weight, at::Tensor bias,
                                   OptTensor running_mean, OptTensor running_var, double momentum, double eps,
                                   bool training, bool relu, OptTensor num_batches, OptTensor sums, OptTensor res_coef,
                                   bool apply, OptTensor out, c10::optional<std::vector<at::Tensor>> pre) {
    const char *op = "bn_forward";
    auto sh = bn_shape(x, op);
    const int C = sh.channels;
    const Dev dev = x.device();
    kfk::BnForwardArgs a;
    a.bn = bn_common(op, sh, dev, weight, bias, running_mean, running_var, num_batches, training, momentum, eps);
    a.x = bf16(x), a.training = training, a.relu = relu, a.apply = apply;
    if (has(res)) {
        check_cl4(*res, op, "res", dev, x.sizes());
        a.res = bf16(*res);
    }
    if (has(res_coef)) {
        TORCH_CHECK(a.res, "bn_forward: res_coef (the residual BN's f32 [scale(C); shift(C)]) needs res");
        check_dense(*res_coef, op, "res_coef", dev, at::kFloat, 2 * C);
        a.res_coef = res_coef->data_ptr<float>();
    }
    if (has(out)) {
        // a channel slice [N, C, H, W] of a wider channels_last bf16 tensor (a concatenation)
        TORCH_CHECK(apply && !a.res && relu && out->scalar_type() == at::kBFloat16 && out->sizes() == x.sizes() &&
                        out->stride(1) == 1 && out->stride(3) >= C && out->stride(3) % 8 == 0 &&
                        out->stride(2) == out->size(3) * out->stride(3) &&
                        out->stride(0) == out->size(2) * out->stride(2) &&
                        reinterpret_cast<uintptr_t>(out->data_ptr()) % 16 == 0 && out->device() == x.device(),
                    "bn_forward: out must be a 16-byte aligned channel slice of a channels_last bf16 tensor "
                    "(BN+ReLU, no residual)");
        a.y_ld = out->stride(3);
    }
    a.prefinalized = pre.has_value();
    if (a.prefinalized) {
        // (mean, invstd, coef) already written from `sums` by the batched bn_finalize_multi launch
        TORCH_CHECK(pre->size() == 3 && training && has(sums), "bn_forward: pre must be (mean, invstd, coef) with sums");
        check_dense((*pre)[0], op, "pre[0]", dev, at::kFloat, C);
        check_dense((*pre)[1], op, "pre[1]", dev, at::kFloat, C);
        check_dense((*pre)[2], op, "pre[2]", dev, at::kFloat, 2 * C);
    }
    if (training) a.bn.sums = stats_ptr(sums, op, C, dev, "sums");

    c10::DeviceGuard gd(x.device());
    auto fopt = x.options().dtype(at::kFloat);
    at::Tensor y;
    if (has(out)) y = *out;
    else if (apply) y = at::empty_like(x, kCL);
    if (apply) a.y = bf16_mut(y);
    const std::vector<at::Tensor> st = a.prefinalized ? *pre : alloc_stats(C, fopt);
    out_stats(a.bn, st);
    at::Tensor mask;
    if (apply && a.res && relu) {
        mask = at::empty({sh.rows * (C / 8)}, x.options().dtype(at::kByte));
        a.mask = mask.data_ptr<uint8_t>();
    }
    at::Tensor partial;
    if (training && !a.bn.sums) {
        partial = alloc_partial(sh, fopt);
        a.bn.partial = partial.data_ptr<float>();
    }
    kfk::launch_bn_forward(a, stream_of(x, 0));
    return {y, st[0], st[1], st[2], mask};
}

// Returns (dx, dres or undefined, dweight, dbias).
std::vector<at::Tensor> bn_backward(at::Tensor dy, at::Tensor x, at::Tensor mean, at::Tensor invstd, at::Tensor weight,
                                    at::Tensor fcoef, OptTensor mask, bool relu, bool training, bool want_dres,
                                    OptTensor sums, OptTensor dres_x, OptTensor dres_sums) {
    const char *op = "bn_backward";
    auto sh = bn_shape(x, op);
    const int C = sh.channels;
    const Dev dev = x.device();
    check_bn_dy(dy, x, op);
    kfk::BnBackwardArgs a;
    a.bn = bn_saved(op, sh, dev, mean, invstd, weight, fcoef);
    a.bn.training = training;
    a.x = bf16(x), a.fcoef = fcoef.data_ptr<float>(), a.relu = relu;
    if (has(mask)) {
        check_dense(*mask, op, "mask", dev, at::kByte, sh.rows * (C / 8));
        a.mask = mask->data_ptr<uint8_t>();
    }
    a.bn.sums = stats_ptr(sums, op, C, dev, "sums");
    if (has(dres_x)) {
        TORCH_CHECK(want_dres && has(dres_sums),
                    "bn_backward: dres_x (second BN's input) needs want_dres and its f64 sums workspace dres_sums");
        check_cl4(*dres_x, op, "dres_x", dev, x.sizes());
        a.dres_x = bf16(*dres_x);
        a.dres_sums = stats_ptr(dres_sums, op, C, dev, "dres_sums");
    }
    c10::DeviceGuard gd(x.device());
    dy = bn_dy(dy, x, C, &a.dy_ld);
    a.dy = bf16(dy);
    auto fopt = x.options().dtype(at::kFloat);
    auto dx = at::empty_like(x, kCL);
    a.dx = bf16_mut(dx);
    at::Tensor dres;
    if (want_dres) {
        dres = at::empty_like(x, kCL);
        a.dres = bf16_mut(dres);
    }
    const auto o = alloc_bwd_out(a.bn, fopt);
    at::Tensor partial;
    if (!a.bn.sums) {
        partial = alloc_partial(sh, fopt);
        a.bn.partial = partial.data_ptr<float>();
    }
    kfk::launch_bn_backward(a, stream_of(x, 0));
    return {dx, dres, o[0], o[1]};
}

// Backward of several training BN+ReLUs (no residual, no sums) whose output gradients may be channel
// slices of one concatenation's gradient: every reduce pass, ONE batched finalize, every apply pass.
// Returns [dx, dgamma, dbeta] per BN.
std::vector<std::vector<at::Tensor>> bn_backward_multi(std::vector<at::Tensor> dys, std::vector<at::Tensor> xs,
                                                       std::vector<at::Tensor> means, std::vector<at::Tensor> invstds,
                                                       std::vector<at::Tensor> weights, std::vector<at::Tensor> fcoefs) {
    const char *op = "bn_backward_multi";
    const size_t n = xs.size();
    TORCH_CHECK(n >= 1 && n <= static_cast<size_t>(kfk::kBnFinMax) && dys.size() == n && means.size() == n &&
                    invstds.size() == n && weights.size() == n && fcoefs.size() == n,
                "bn_backward_multi: 1..8 BNs, every list of the same length");
    std::vector<kfk::BnBackwardArgs> as(n);
    std::vector<kfk::BNShape> shs(n);
    const Dev dev = xs[0].device();
    for (size_t i = 0; i < n; ++i) {
        shs[i] = bn_shape(xs[i], op);
        TORCH_CHECK(xs[i].device() == *dev, "bn_backward_multi: xs must be on one device");
        check_bn_dy(dys[i], xs[i], op);
        as[i].bn = bn_saved(op, shs[i], dev, means[i], invstds[i], weights[i], fcoefs[i], "s");
        as[i].x = bf16(xs[i]), as[i].fcoef = fcoefs[i].data_ptr<float>(), as[i].relu = true;
    }
    c10::DeviceGuard gd(xs[0].device());
    std::vector<at::Tensor> keep;  // the gradients read (a copy where bn_dy made one) and the partials
    std::vector<std::vector<at::Tensor>> out;
    kfk::BnBwdFinBatch fb{};
    fb.n = static_cast<int>(n);
    for (size_t i = 0; i < n; ++i) {
        kfk::BnBackwardArgs &a = as[i];
        auto fopt = xs[i].options().dtype(at::kFloat);
        keep.push_back(bn_dy(dys[i], xs[i], a.bn.C, &a.dy_ld));
        a.dy = bf16(keep.back());
        auto dx = at::empty_like(xs[i], kCL);
        a.dx = bf16_mut(dx);
        const auto o = alloc_bwd_out(a.bn, fopt);
        keep.push_back(alloc_partial(shs[i], fopt));
        a.bn.partial = keep.back().data_ptr<float>();
        fb.d[i] = a.bn;
        out.push_back({dx, o[0], o[1]});
        keep.push_back(o[2]);
    }
    const hipStream_t st = stream_of(xs[0], 0);
    for (auto &a : as) kfk::launch_bn_backward_reduce(a, st);
    kfk::launch_bn_bwd_finalize_multi(fb, st);
    for (auto &a : as) kfk::launch_bn_backward_apply(a, st);
    return out;
}

// Stem BN+ReLU+MaxPool(3,2,1).  Returns (y_pool, mean, invstd, coef, argmax bytes).
std::vector<at::Tensor> bn_pool_forward(at::Tensor x, at::Tensor weight, at::Tensor bias, OptTensor running_mean,
                                        OptTensor running_var, double momentum, double eps, bool training,
                                        OptTensor num_batches, OptTensor sums) {
    const char *op = "bn_pool_forward";
    auto sh = bn_shape(x, op);
    const int C = sh.channels;
    const Dev dev = x.device();
    kfk::BnPoolForwardArgs a;
    a.H = narrow(x.size(2), op, "x"), a.W = narrow(x.size(3), op, "x");
    TORCH_CHECK(kfk::bn_pool_supported(sh, a.H, a.W), "bn_pool_forward: unsupported shape");
    double *sp = training ? stats_ptr(sums, op, C, dev, "sums") : nullptr;
    a.bn = bn_common(op, sh, dev, weight, bias, running_mean, running_var, num_batches, training, momentum, eps);
    a.bn.sums = sp;
    a.x = bf16(x), a.training = training;
    c10::DeviceGuard gd(x.device());
    auto fopt = x.options().dtype(at::kFloat);
    const int OH = kfk::pool_out(a.H), OW = kfk::pool_out(a.W);
    auto yp = at::empty({x.size(0), C, OH, OW}, x.options().memory_format(kCL));
    auto arg = at::empty({x.size(0) * OH * OW * C}, x.options().dtype(at::kByte));
    a.yp = bf16_mut(yp), a.arg = arg.data_ptr<uint8_t>();
    const auto st = alloc_stats(C, fopt);
    out_stats(a.bn, st);
    at::Tensor partial, xarg;
    if (training) {
        partial = alloc_partial(sh, fopt);
        xarg = at::empty_like(yp, kCL);
        a.bn.partial = partial.data_ptr<float>(), a.xarg = bf16_mut(xarg);
    }
    kfk::launch_bn_pool_forward(a, stream_of(x, 0));
    return {yp, st[0], st[1], st[2], arg, xarg};
}

// Returns (dx, dweight, dbias).
std::vector<at::Tensor> bn_pool_backward(at::Tensor dyp, at::Tensor arg, at::Tensor x, at::Tensor mean,
                                         at::Tensor invstd, at::Tensor weight, at::Tensor fcoef, bool training,
                                         OptTensor xarg, bool apply) {
    const char *op = "bn_pool_backward";
    auto sh = bn_shape(x, op);
    const int C = sh.channels;
    const Dev dev = x.device();
    kfk::BnPoolBackwardArgs a;
    a.H = narrow(x.size(2), op, "x"), a.W = narrow(x.size(3), op, "x");
    const int64_t psz[4] = {x.size(0), C, kfk::pool_out(a.H), kfk::pool_out(a.W)};
    TORCH_CHECK(dyp.scalar_type() == at::kBFloat16 && dyp.sizes() == at::IntArrayRef(psz) && dyp.device() == x.device(),
                "bn_pool_backward: dy must be the pooled [N, C, PH, PW] bf16 gradient on x's device");
    check_dense(arg, op, "arg", dev, at::kByte, dyp.numel());
    a.bn = bn_saved(op, sh, dev, mean, invstd, weight, fcoef);
    a.bn.training = training;
    a.arg = arg.data_ptr<uint8_t>(), a.x = bf16(x), a.fcoef = fcoef.data_ptr<float>(), a.apply = apply;
    const bool pooled = training && has(xarg);
    if (pooled) {
        check_cl4(*xarg, op, "xarg", dev, psz);
        a.xarg = bf16(*xarg);
    }
    c10::DeviceGuard gd(x.device());
    if (!dyp.is_contiguous(kCL)) dyp = dyp.contiguous(kCL);
    a.dyp = bf16(dyp);
    auto fopt = x.options().dtype(at::kFloat);
    // apply = false: statistics + finalize only -- dx is not formed (an empty tensor), the backward
    // coefficients [k1; k2; k3] are returned for the caller's own pass (stem_wgrad_bnp)
    auto dx = apply ? at::empty_like(x, kCL) : at::empty({0}, x.options());
    if (apply) a.dx = bf16_mut(dx);
    const auto o = alloc_bwd_out(a.bn, fopt);
    auto partial = alloc_partial(sh, fopt);
    a.bn.partial = partial.data_ptr<float>();
    at::Tensor sums;
    if (pooled) {
        sums = at::zeros({2 * C * kfk::kStatSlots}, x.options().dtype(at::kDouble));
        a.bn.sums = sums.data_ptr<double>();
    }
    kfk::launch_bn_pool_backward(a, stream_of(x, 0));
    return {dx, o[0], o[1], o[2]};
}

}  // namespace

void bind_bn(py::module_ &m) {
    m.def("bn_supported_channels", &kfk::bn_supported_channels);
    m.def("bn_forward", &bn_forward,
          "fused NHWC BN(+residual)(+ReLU) forward -> (y, mean, invstd, coef, relu mask or None)", py::arg("x"),
          py::arg("res"), py::arg("weight"), py::arg("bias"), py::arg("running_mean"), py::arg("running_var"),
          py::arg("momentum"), py::arg("eps"), py::arg("training"), py::arg("relu"),
          py::arg("num_batches") = py::none(), py::arg("sums") = py::none(), py::arg("res_coef") = py::none(),
          py::arg("apply") = true, py::arg("out") = py::none(), py::arg("pre") = py::none());
    m.def("bn_backward_multi", &bn_backward_multi,
          "backward of several BN+ReLUs (slices of one concatenation's gradient): one batched finalize");
    m.def("bn_finalize_multi", &bn_finalize_multi,
          "batched sums-finalize of several training BNs in one launch -> [[mean, invstd, coef], ...]");
    m.def("bn_backward", &bn_backward, "fused NHWC BN(+residual)(+ReLU) backward -> (dx, dres, dweight, dbias)",
          py::arg("dy"), py::arg("x"), py::arg("mean"), py::arg("invstd"), py::arg("weight"), py::arg("fcoef"),
          py::arg("mask"), py::arg("relu"), py::arg("training"), py::arg("want_dres"), py::arg("sums") = py::none(),
          py::arg("dres_x") = py::none(), py::arg("dres_sums") = py::none());
    m.def("bn_pool_supported", [](int64_t C, int64_t H, int64_t W) {
        const char *op = "bn_pool_supported";
        return kfk::bn_pool_supported(kfk::BNShape{H * W, narrow(C, op, "C")}, narrow(H, op, "H"), narrow(W, op, "W"));
    });
    m.def("bn_pool_forward", &bn_pool_forward,
          "stem BN+ReLU+MaxPool(3,2,1) forward -> (y_pool, mean, invstd, coef, argmax)", py::arg("x"),
          py::arg("weight"), py::arg("bias"), py::arg("running_mean"), py::arg("running_var"), py::arg("momentum"),
          py::arg("eps"), py::arg("training"), py::arg("num_batches") = py::none(), py::arg("sums") = py::none());
    m.def("bn_pool_backward", &bn_pool_backward, "stem BN+ReLU+MaxPool backward -> (dx, dweight, dbias, coef)",
          py::arg("dy"), py::arg("arg"), py::arg("x"), py::arg("mean"), py::arg("invstd"), py::arg("weight"),
          py::arg("fcoef"), py::arg("training"), py::arg("xarg") = py::none(), py::arg("apply") = true);
}
