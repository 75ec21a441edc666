// Fused NHWC BatchNorm (+residual, +ReLU, +MaxPool) forward / backward.
#include "bind_util.hpp"

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

struct BNCommon {
    float *rm = nullptr, *rv = nullptr;
    int64_t *nbt = nullptr;
};

BNCommon bn_common(const char *op, int C, const Dev &dev, const at::Tensor &weight, const at::Tensor &bias,
                   const OptTensor &running_mean, const OptTensor &running_var, const OptTensor &num_batches,
                   bool training) {
    check_dense(weight, op, "weight", dev, at::kFloat, C);
    check_dense(bias, op, "bias", dev, at::kFloat, C);
    BNCommon b;
    if (has(running_mean)) {
        TORCH_CHECK(has(running_var), op, ": running_var missing");
        b.rm = running_mean->data_ptr<float>();
        b.rv = running_var->data_ptr<float>();
    }
    TORCH_CHECK(training || b.rm, op, ": eval mode needs running stats");
    if (training && has(num_batches)) {
        TORCH_CHECK(num_batches->scalar_type() == at::kLong && num_batches->numel() == 1 && num_batches->is_cuda(),
                    op, ": num_batches_tracked must be a 1-element int64 GPU tensor");
        b.nbt = num_batches->data_ptr<int64_t>();
    }
    return b;
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
    for (size_t i = 0; i < n; ++i) {
        auto sh = bn_shape(xs[i], op);
        const Dev dev = xs[0].device();
        TORCH_CHECK(xs[i].device() == *dev, "bn_finalize_multi: xs must be on one device");
        auto c = bn_common(op, sh.channels, dev, weights[i], biases[i], running_means[i], running_vars[i],
                           num_batches[i], true);
        kfk::BnFinDesc &d = b.d[i];
        TORCH_CHECK(sums[i].defined(), "bn_finalize_multi: sums must be defined");
        d.sums = stats_ptr(sums[i], op, sh.channels, dev, "sums");
        d.gamma = weights[i].data_ptr<float>(), d.beta = biases[i].data_ptr<float>();
        d.run_mean = c.rm, d.run_var = c.rv, d.nbt = c.nbt;
        d.rows = sh.rows, d.C = sh.channels;
        d.momentum = static_cast<float>(momentum[i]), d.eps = static_cast<float>(eps[i]);
    }
    std::vector<std::vector<at::Tensor>> out;
    for (size_t i = 0; i < n; ++i) {
        kfk::BnFinDesc &d = b.d[i];
        auto fopt = xs[i].options().dtype(at::kFloat);
        at::Tensor mean = at::empty({d.C}, fopt), invstd = at::empty({d.C}, fopt), coef = at::empty({2 * d.C}, fopt);
        d.mean = mean.data_ptr<float>(), d.invstd = invstd.data_ptr<float>(), d.coef = coef.data_ptr<float>();
        out.push_back({mean, invstd, coef});
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
    auto b = bn_common(op, C, dev, weight, bias, running_mean, running_var, num_batches, training);
    const uint16_t *rp = nullptr;
    if (has(res)) {
        check_cl4(*res, op, "res", dev, x.sizes());
        rp = bf16(*res);
    }
    const float *rc = nullptr;
    if (has(res_coef)) {
        TORCH_CHECK(rp, "bn_forward: res_coef (the residual BN's f32 [scale(C); shift(C)]) needs res");
        check_dense(*res_coef, op, "res_coef", dev, at::kFloat, 2 * C);
        rc = res_coef->data_ptr<float>();
    }
    int64_t y_ld = 0;
    if (has(out)) {
        // a channel slice [N, C, H, W] of a wider channels_last bf16 tensor (a concatenation)
        TORCH_CHECK(apply && !rp && relu && out->scalar_type() == at::kBFloat16 && out->sizes() == x.sizes() &&
                        out->stride(1) == 1 && out->stride(3) >= C && out->stride(3) % 8 == 0 &&
                        out->stride(2) == out->size(3) * out->stride(3) &&
                        out->stride(0) == out->size(2) * out->stride(2) &&
                        reinterpret_cast<uintptr_t>(out->data_ptr()) % 16 == 0 && out->device() == x.device(),
                    "bn_forward: out must be a 16-byte aligned channel slice of a channels_last bf16 tensor "
                    "(BN+ReLU, no residual)");
        y_ld = out->stride(3);
    }
    const bool prefin = pre.has_value();
    if (prefin) {
        // (mean, invstd, coef) already written from `sums` by the batched bn_finalize_multi launch
        TORCH_CHECK(pre->size() == 3 && training && has(sums), "bn_forward: pre must be (mean, invstd, coef) with sums");
        check_dense((*pre)[0], op, "pre[0]", dev, at::kFloat, C);
        check_dense((*pre)[1], op, "pre[1]", dev, at::kFloat, C);
        check_dense((*pre)[2], op, "pre[2]", dev, at::kFloat, 2 * C);
    }
    double *sp = training ? stats_ptr(sums, op, C, dev, "sums") : nullptr;

    c10::DeviceGuard gd(x.device());
    auto fopt = x.options().dtype(at::kFloat);
    at::Tensor y;
    if (has(out)) y = *out;
    else if (apply) y = at::empty_like(x, kCL);
    at::Tensor mean, invstd, coef;
    if (prefin) mean = (*pre)[0], invstd = (*pre)[1], coef = (*pre)[2];
    else mean = at::empty({C}, fopt), invstd = at::empty({C}, fopt), coef = at::empty({2 * C}, fopt);
    at::Tensor mask;
    if (apply && rp && relu) mask = at::empty({sh.rows * (C / 8)}, x.options().dtype(at::kByte));
    at::Tensor partial;
    if (training && !sp) partial = at::empty({2 * static_cast<int64_t>(kfk::bn_num_chunks(sh)) * C}, fopt);
    kfk::launch_bn_forward(bf16(x), rp, weight.data_ptr<float>(), bias.data_ptr<float>(),
                           apply ? bf16_mut(y) : nullptr, mask.defined() ? mask.data_ptr<uint8_t>() : nullptr, sh, relu,
                           training, b.rm, b.rv, static_cast<float>(momentum), static_cast<float>(eps),
                           partial.defined() ? partial.data_ptr<float>() : nullptr, mean.data_ptr<float>(),
                           invstd.data_ptr<float>(), coef.data_ptr<float>(), b.nbt, stream_of(x, 0), sp, rc, apply, y_ld,
                           prefin);
    return {y, mean, invstd, coef, mask};
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
    check_dense(mean, op, "mean", dev, at::kFloat, C);
    check_dense(invstd, op, "invstd", dev, at::kFloat, C);
    check_dense(weight, op, "weight", dev, at::kFloat, C);
    check_dense(fcoef, op, "fcoef", dev, at::kFloat, 2 * C);
    const uint8_t *mp = nullptr;
    if (has(mask)) {
        check_dense(*mask, op, "mask", dev, at::kByte, sh.rows * (C / 8));
        mp = mask->data_ptr<uint8_t>();
    }
    double *sp = stats_ptr(sums, op, C, dev, "sums");
    const uint16_t *dsx = nullptr;
    double *dsp = nullptr;
    if (has(dres_x)) {
        TORCH_CHECK(want_dres && has(dres_sums),
                    "bn_backward: dres_x (second BN's input) needs want_dres and its f64 sums workspace dres_sums");
        check_cl4(*dres_x, op, "dres_x", dev, x.sizes());
        dsx = bf16(*dres_x);
        dsp = stats_ptr(dres_sums, op, C, dev, "dres_sums");
    }
    c10::DeviceGuard gd(x.device());
    int64_t dy_ld;
    dy = bn_dy(dy, x, C, &dy_ld);
    auto fopt = x.options().dtype(at::kFloat);
    auto dx = at::empty_like(x, kCL);
    at::Tensor dres;
    if (want_dres) dres = at::empty_like(x, kCL);
    at::Tensor dw = at::empty({C}, fopt), db = at::empty({C}, fopt), coef = at::empty({3 * C}, fopt);
    at::Tensor partial;
    if (!sp) partial = at::empty({2 * static_cast<int64_t>(kfk::bn_num_chunks(sh)) * C}, fopt);
    kfk::launch_bn_backward(bf16(dy), bf16(x), fcoef.data_ptr<float>(), mp, mean.data_ptr<float>(),
                            invstd.data_ptr<float>(), weight.data_ptr<float>(), sh, relu, training,
                            partial.defined() ? partial.data_ptr<float>() : nullptr, dw.data_ptr<float>(),
                            db.data_ptr<float>(), coef.data_ptr<float>(), bf16_mut(dx),
                            want_dres ? bf16_mut(dres) : nullptr, stream_of(x, 0), sp, dsx, dsp, dy_ld);
    return {dx, dres, dw, db};
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
    struct Piece {
        at::Tensor dy, dx, dw, db, coef, partial;
        int64_t ld;
        kfk::BNShape sh;
    };
    std::vector<Piece> ps(n);
    const Dev dev = xs[0].device();
    for (size_t i = 0; i < n; ++i) {
        ps[i].sh = bn_shape(xs[i], op);
        const int C = ps[i].sh.channels;
        TORCH_CHECK(xs[i].device() == *dev, "bn_backward_multi: xs must be on one device");
        check_bn_dy(dys[i], xs[i], op);
        check_dense(fcoefs[i], op, "fcoefs", dev, at::kFloat, 2 * C);
        check_dense(means[i], op, "means", dev, at::kFloat, C);
        check_dense(invstds[i], op, "invstds", dev, at::kFloat, C);
        check_dense(weights[i], op, "weights", dev, at::kFloat, C);
    }
    c10::DeviceGuard gd(xs[0].device());
    kfk::BnBwdFinBatch fb{};
    fb.n = static_cast<int>(n);
    for (size_t i = 0; i < n; ++i) {
        Piece &p = ps[i];
        const int C = p.sh.channels;
        p.dy = bn_dy(dys[i], xs[i], C, &p.ld);
        auto fopt = xs[i].options().dtype(at::kFloat);
        p.dx = at::empty_like(xs[i], kCL);
        p.dw = at::empty({C}, fopt), p.db = at::empty({C}, fopt), p.coef = at::empty({3 * C}, fopt);
        p.partial = at::empty({2 * static_cast<int64_t>(kfk::bn_num_chunks(p.sh)) * C}, fopt);
        kfk::BnBwdFinDesc &d = fb.d[i];
        d.partial = p.partial.data_ptr<float>();
        d.nchunks = kfk::bn_num_chunks(p.sh), d.C = C, d.rows = p.sh.rows;
        d.gamma = weights[i].data_ptr<float>(), d.mean = means[i].data_ptr<float>(), d.invstd = invstds[i].data_ptr<float>();
        d.dgamma = p.dw.data_ptr<float>(), d.dbeta = p.db.data_ptr<float>(), d.coef = p.coef.data_ptr<float>();
    }
    const hipStream_t st = stream_of(xs[0], 0);
    for (int phase : {1, 2}) {
        if (phase == 2) kfk::launch_bn_bwd_finalize_multi(fb, st);
        for (size_t i = 0; i < n; ++i) {
            Piece &p = ps[i];
            kfk::launch_bn_backward(bf16(p.dy), bf16(xs[i]), fcoefs[i].data_ptr<float>(), nullptr,
                                    means[i].data_ptr<float>(), invstds[i].data_ptr<float>(),
                                    weights[i].data_ptr<float>(), p.sh, true, true, p.partial.data_ptr<float>(),
                                    p.dw.data_ptr<float>(), p.db.data_ptr<float>(), p.coef.data_ptr<float>(),
                                    bf16_mut(p.dx), nullptr, st, nullptr, nullptr, nullptr, p.ld, phase);
        }
    }
    std::vector<std::vector<at::Tensor>> out;
    for (auto &p : ps) out.push_back({p.dx, p.dw, p.db});
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
    const int H = narrow(x.size(2), op, "x"), W = narrow(x.size(3), op, "x");
    TORCH_CHECK(kfk::bn_pool_supported(sh, H, W), "bn_pool_forward: unsupported shape");
    double *sp = training ? stats_ptr(sums, op, C, dev, "sums") : nullptr;
    auto b = bn_common(op, C, dev, weight, bias, running_mean, running_var, num_batches, training);
    c10::DeviceGuard gd(x.device());
    auto fopt = x.options().dtype(at::kFloat);
    const int OH = kfk::pool_out(H), OW = kfk::pool_out(W);
    auto yp = at::empty({x.size(0), C, OH, OW}, x.options().memory_format(kCL));
    auto arg = at::empty({x.size(0) * OH * OW * C}, x.options().dtype(at::kByte));
    auto mean = at::empty({C}, fopt), invstd = at::empty({C}, fopt), coef = at::empty({2 * C}, fopt);
    at::Tensor partial, xarg;
    if (training) {
        partial = at::empty({2 * static_cast<int64_t>(kfk::bn_num_chunks(sh)) * C}, fopt);
        xarg = at::empty_like(yp, kCL);
    }
    kfk::launch_bn_pool_forward(bf16(x), weight.data_ptr<float>(), bias.data_ptr<float>(), bf16_mut(yp),
                                arg.data_ptr<uint8_t>(), sh, H, W, training, b.rm, b.rv, static_cast<float>(momentum),
                                static_cast<float>(eps), training ? partial.data_ptr<float>() : nullptr,
                                mean.data_ptr<float>(), invstd.data_ptr<float>(), coef.data_ptr<float>(), b.nbt,
                                stream_of(x, 0), sp, xarg.defined() ? bf16_mut(xarg) : nullptr);
    return {yp, mean, invstd, coef, arg, xarg};
}

// Returns (dx, dweight, dbias).
std::vector<at::Tensor> bn_pool_backward(at::Tensor dyp, at::Tensor arg, at::Tensor x, at::Tensor mean,
                                         at::Tensor invstd, at::Tensor weight, at::Tensor fcoef, bool training,
                                         OptTensor xarg, bool apply) {
    const char *op = "bn_pool_backward";
    auto sh = bn_shape(x, op);
    const int C = sh.channels;
    const Dev dev = x.device();
    const int H = narrow(x.size(2), op, "x"), W = narrow(x.size(3), op, "x");
    const int64_t psz[4] = {x.size(0), C, kfk::pool_out(H), kfk::pool_out(W)};
    TORCH_CHECK(dyp.scalar_type() == at::kBFloat16 && dyp.sizes() == at::IntArrayRef(psz) && dyp.device() == x.device(),
                "bn_pool_backward: dy must be the pooled [N, C, PH, PW] bf16 gradient on x's device");
    check_dense(arg, op, "arg", dev, at::kByte, dyp.numel());
    check_dense(mean, op, "mean", dev, at::kFloat, C);
    check_dense(invstd, op, "invstd", dev, at::kFloat, C);
    check_dense(weight, op, "weight", dev, at::kFloat, C);
    check_dense(fcoef, op, "fcoef", dev, at::kFloat, 2 * C);
    const bool pooled = training && has(xarg);
    if (pooled) check_cl4(*xarg, op, "xarg", dev, psz);
    c10::DeviceGuard gd(x.device());
    if (!dyp.is_contiguous(kCL)) dyp = dyp.contiguous(kCL);
    auto fopt = x.options().dtype(at::kFloat);
    // apply = false: statistics + finalize only -- dx is not formed (an empty tensor), the backward
    // coefficients [k1; k2; k3] are returned for the caller's own pass (stem_wgrad_bnp)
    auto dx = apply ? at::empty_like(x, kCL) : at::empty({0}, x.options());
    auto dw = at::empty({C}, fopt), db = at::empty({C}, fopt), coef = at::empty({3 * C}, fopt);
    auto partial = at::empty({2 * static_cast<int64_t>(kfk::bn_num_chunks(sh)) * C}, fopt);
    at::Tensor sums;
    if (pooled) sums = at::zeros({2 * C * kfk::kStatSlots}, x.options().dtype(at::kDouble));
    kfk::launch_bn_pool_backward(bf16(dyp), arg.data_ptr<uint8_t>(), bf16(x), fcoef.data_ptr<float>(),
                                 mean.data_ptr<float>(), invstd.data_ptr<float>(), weight.data_ptr<float>(), sh, H, W,
                                 training, partial.data_ptr<float>(), dw.data_ptr<float>(), db.data_ptr<float>(),
                                 coef.data_ptr<float>(), apply ? bf16_mut(dx) : nullptr, stream_of(x, 0),
                                 pooled ? bf16(*xarg) : nullptr, pooled ? sums.data_ptr<double>() : nullptr, apply);
    return {dx, dw, db, coef};
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
