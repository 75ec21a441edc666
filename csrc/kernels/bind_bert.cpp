// BERT's kernels: cross-entropy, GELU / column sums, attention, LayerNorm, the NT GEMMs.
#include "bind_util.hpp"

#include <tuple>
#include <vector>

using namespace kfb;

namespace {

// fused softmax cross-entropy over bf16 logits [R, V]: (lse [R] f32, per-row loss [R] f32)
// Rows may be padded (x.stride(0) = ld >= V, a multiple of 8, 16-byte aligned base: the vocabulary
// projection's gemm_nt_ld output): the 16-byte-load kernels; those also serve contiguous rows of V % 8 == 0
int64_t xent_ld(const at::Tensor &x) {
    const int64_t ld = x.stride(0), V = x.size(1);
    const bool al = reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0;
    return (x.stride(1) == 1 && ld >= V && ld % 8 == 0 && al) ? ld : 0;
}

void check_logits(const at::Tensor &x, const char *op) {
    TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.dim() == 2 &&
                    (xent_ld(x) > 0 || (x.is_contiguous() && x.size(1) % 2 == 0)),
                op, ": x must be bf16 [R, V] logits, contiguous with V even or rows padded to a multiple of 8");
}

std::vector<at::Tensor> xent_forward(at::Tensor x, at::Tensor labels) {
    const char *op = "xent_forward";
    check_logits(x, op);
    check_dense(labels, op, "labels", x.device(), at::kLong, x.size(0));
    TORCH_CHECK(x.size(1) < (int64_t(1) << 30) && x.size(0) < (int64_t(1) << 31), "xent_forward: shape too large");
    c10::DeviceGuard gd(x.device());
    auto lse = at::empty({x.size(0)}, x.options().dtype(at::kFloat));
    auto loss = at::empty({x.size(0)}, x.options().dtype(at::kFloat));
    kfk::launch_xent_forward(bf16(x), labels.data_ptr<int64_t>(), x.size(0), static_cast<int>(x.size(1)),
                             lse.data_ptr<float>(), loss.data_ptr<float>(), stream_of(x, 0), xent_ld(x));
    return {lse, loss};
}

// its backward: d logits (bf16 [R, V]) = (softmax - onehot(label)) * scale[0]; padded logits give a
// gradient with the same padded row stride (a [R, V] view of [R, ld], the padding of the last chunk zero)
at::Tensor xent_backward(at::Tensor x, at::Tensor labels, at::Tensor lse, at::Tensor scale) {
    const char *op = "xent_backward";
    check_logits(x, op);
    const Dev dev = x.device();
    check_dense(labels, op, "labels", dev, at::kLong, x.size(0));
    TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.numel() == x.size(0) && scale.scalar_type() == at::kFloat &&
                    scale.numel() >= 1 && lse.device() == x.device() && scale.device() == x.device(),
                "xent_backward: lse must be f32 [R] and scale f32 [1] on the logits' device");
    const int V = narrow(x.size(1), op, "V");
    c10::DeviceGuard gd(x.device());
    const int64_t ld = xent_ld(x);
    auto dxp = ld > 0 ? at::empty({x.size(0), ld}, x.options()) : at::empty_like(x);
    kfk::launch_xent_backward(bf16(x), labels.data_ptr<int64_t>(), lse.data_ptr<float>(), scale.data_ptr<float>(),
                              x.size(0), V, bf16_mut(dxp), stream_of(x, 0), ld);
    return ld > 0 && ld != x.size(1) ? dxp.narrow(1, 0, x.size(1)) : dxp;
}

// f32 (out_f32) or bf16 (out_bf16) destination pointers of a column-sum output
struct SumOut {
    float *f32;
    uint16_t *b16;
};
SumOut sum_out(const at::Tensor &t) {
    const bool f = t.scalar_type() == at::kFloat;
    return {f ? t.data_ptr<float>() : nullptr, f ? nullptr : bf16_mut(t)};
}

// GELU backward fused with the bias gradient: (du, colsum(du)) for bf16 dy, u [..., O] (O % 8 == 0).
std::vector<at::Tensor> gelu_backward_colsum(at::Tensor dy, at::Tensor u, at::ScalarType dtype) {
    const char *op = "gelu_backward_colsum";
    check_dense(dy, op, "dy", kAnyGpu, at::kBFloat16, dy.numel());
    check_dense(u, op, "u", dy.device(), at::kBFloat16, dy.numel());
    TORCH_CHECK(u.sizes() == dy.sizes() && dy.numel() > 0 && dy.size(-1) % 8 == 0,
                "gelu_backward_colsum: dy and u must have equal shape, last dim % 8");
    TORCH_CHECK(dtype == at::kFloat || dtype == at::kBFloat16, "gelu_backward_colsum: dtype float32 or bfloat16");
    c10::DeviceGuard gd(dy.device());
    const int O = narrow(dy.size(-1), op, "the last dim");
    const int64_t T = dy.numel() / O;
    auto du = at::empty_like(dy);
    auto part = at::empty({static_cast<int64_t>(kfk::gelu_colsum_chunks(T, O)) * O}, dy.options().dtype(at::kFloat));
    auto out = at::empty({O}, dy.options().dtype(dtype));
    const auto so = sum_out(out);
    kfk::launch_gelu_bwd_colsum(bf16(dy), bf16(u), bf16_mut(du), T, O, part.data_ptr<float>(), so.f32, so.b16,
                                stream_of(dy, 0));
    return {du, out};
}

// Column sums of a contiguous bf16 [T, O] (O % 8 == 0) -> [O] in `dtype` (f32 or bf16).
at::Tensor colsum(at::Tensor x, at::ScalarType dtype) {
    const char *op = "colsum";
    check_dense(x, op, "x", kAnyGpu, at::kBFloat16, x.numel());
    TORCH_CHECK(x.dim() == 2 && x.size(1) % 8 == 0 && x.size(0) > 0, "colsum: x must be [T, O] with O % 8 == 0");
    TORCH_CHECK(dtype == at::kFloat || dtype == at::kBFloat16, "colsum: dtype must be float32 or bfloat16");
    c10::DeviceGuard gd(x.device());
    const int64_t T = x.size(0);
    const int O = narrow(x.size(1), op, "O");
    auto part = at::empty({static_cast<int64_t>(kfk::colsum_chunks(T, O)) * O}, x.options().dtype(at::kFloat));
    auto out = at::empty({O}, x.options().dtype(dtype));
    const auto so = sum_out(out);
    kfk::launch_colsum_bf16(bf16(x), T, O, part.data_ptr<float>(), so.f32, so.b16, stream_of(x, 0));
    return out;
}

// contiguous bf16 [B, S, 3*H*64] with S a multiple of 64 up to 512: {B, S, H}
// (stream_kernel, the streaming kernels at S = 128 for tests, is refused where they do not exist: S = 64)
std::tuple<int, int, int> check_qkv(const at::Tensor &qkv, int64_t heads, const char *op, bool stream_kernel) {
    check_dense(qkv, op, "qkv", kAnyGpu, at::kBFloat16, qkv.numel());
    TORCH_CHECK(qkv.dim() == 3 && qkv.size(2) == 3 * heads * 64 && kfk::attention_supported(qkv.size(1), 64), op,
                ": qkv must be [B, S, 3*H*64] with S ", kfk::kAttentionLengths);
    TORCH_CHECK(!stream_kernel || qkv.size(1) >= 128, op, ": stream_kernel needs S >= 128");
    return {narrow(qkv.size(0), op, "B"), narrow(qkv.size(1), op, "S"), narrow(heads, op, "heads")};
}

// Fused self-attention: qkv [B, S, 3*H*64] bf16 contiguous -> (out [B, S, H*64] bf16, lse [B, H, S] f32)
// stream_kernel: S = 128 on the streaming kernels of attention_long.hip (S > 128 always runs them)
std::vector<at::Tensor> attention_forward(at::Tensor qkv, int64_t heads, double scale, int64_t seed, double p_drop,
                                          bool stream_kernel) {
    const auto [B, S, H] = check_qkv(qkv, heads, "attention_forward", stream_kernel);
    c10::DeviceGuard gd(qkv.device());
    auto out = at::empty({B, S, H * 64}, qkv.options());
    auto lse = at::empty({B, H, S}, qkv.options().dtype(at::kFloat));
    kfk::launch_attention_forward(bf16(qkv), bf16_mut(out), lse.data_ptr<float>(), B, S, H, static_cast<float>(scale),
                                  static_cast<uint32_t>(seed), static_cast<float>(p_drop), stream_of(qkv, 0),
                                  stream_kernel);
    return {out, lse};
}

at::Tensor attention_backward(at::Tensor qkv, at::Tensor out, at::Tensor lse, at::Tensor dout, int64_t heads,
                              double scale, int64_t seed, double p_drop, bool stream_kernel) {
    const char *op = "attention_backward";
    const auto [B, S, H] = check_qkv(qkv, heads, op, stream_kernel);
    const Dev dev = qkv.device();
    check_dense(out, op, "out", dev, at::kBFloat16, out.numel());
    TORCH_CHECK(out.sizes() == at::IntArrayRef({B, S, H * 64}),
                "attention_backward: out must be the forward's [B, S, H*64] output");
    TORCH_CHECK(dout.sizes() == out.sizes() && dout.scalar_type() == at::kBFloat16 && dout.device() == qkv.device(),
                "attention_backward: dout must be bf16 of out's shape on qkv's device");
    check_dense(lse, op, "lse", dev, at::kFloat, lse.numel());
    TORCH_CHECK(lse.sizes() == at::IntArrayRef({B, H, S}), "attention_backward: lse must be the forward's [B, H, S] f32");
    c10::DeviceGuard gd(qkv.device());
    if (!dout.is_contiguous()) dout = dout.contiguous();
    auto dqkv = at::empty_like(qkv);
    // rowsum(dO o O): the streaming dQ kernel fills it for the dK/dV kernel
    at::Tensor dsum;
    if (S > 128 || stream_kernel) dsum = at::empty({B, H, S}, lse.options());
    kfk::launch_attention_backward(bf16(qkv), bf16(out), lse.data_ptr<float>(), bf16(dout), bf16_mut(dqkv), B, S, H,
                                   static_cast<float>(scale), static_cast<uint32_t>(seed), static_cast<float>(p_drop),
                                   stream_of(qkv, 0), dsum.defined() ? dsum.data_ptr<float>() : nullptr, stream_kernel);
    return dqkv;
}

// y, s, mean, rstd = layernorm(x [+ r]) over the last dim (bf16 rows, f32 affine)
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> layernorm_forward(at::Tensor x, OptTensor r, at::Tensor gamma,
                                                                             at::Tensor beta, double eps, double p,
                                                                             int64_t seed) {
    const char *op = "layernorm_forward";
    check_dense(x, op, "x", kAnyGpu, at::kBFloat16, x.numel());
    const Dev dev = x.device();
    const int D = narrow(x.size(-1), op, "the row length");
    TORCH_CHECK(kfk::layernorm_supported(D), "layernorm_forward: unsupported row length ", D);
    check_dense(gamma, op, "gamma", dev, at::kFloat, D);
    check_dense(beta, op, "beta", dev, at::kFloat, D);
    const uint16_t *rp = nullptr;
    if (has(r)) {
        check_dense(*r, op, "r", dev, at::kBFloat16, x.numel());
        TORCH_CHECK(r->sizes() == x.sizes(), "layernorm_forward: r must match x");
        rp = bf16(*r);
    }
    c10::DeviceGuard gd(x.device());
    const int64_t rows = x.numel() / D;
    auto y = at::empty_like(x);
    auto sv = rp ? at::empty_like(x) : x;
    auto mean = at::empty({rows}, x.options().dtype(at::kFloat));
    auto rstd = at::empty({rows}, x.options().dtype(at::kFloat));
    kfk::launch_layernorm_forward(bf16(x), rp, gamma.data_ptr<float>(), beta.data_ptr<float>(), bf16_mut(y),
                                  rp ? bf16_mut(sv) : nullptr, mean.data_ptr<float>(), rstd.data_ptr<float>(), rows, D,
                                  static_cast<float>(eps), stream_of(x, 0), static_cast<float>(p),
                                  static_cast<uint32_t>(seed));
    return {y, sv, mean, rstd};
}

// Returns (ds, dgamma, dbeta, dr): dr (p > 0 only, else undefined) is the gradient of the dropped
// residual input.
// rbias_dtype (float32 / bfloat16, optional): also return the column sums of the residual input's
// gradient (dr, or ds without dropout) in that dtype -- the bias gradient of the linear layer that
// produced the residual input.
std::vector<at::Tensor> layernorm_backward(at::Tensor dy, at::Tensor s, at::Tensor gamma, at::Tensor mean,
                                           at::Tensor rstd, double p, int64_t seed,
                                           c10::optional<at::ScalarType> rbias_dtype) {
    const char *op = "layernorm_backward";
    check_dense(dy, op, "dy", kAnyGpu, at::kBFloat16, dy.numel());
    const Dev dev = dy.device();
    check_dense(s, op, "s", dev, at::kBFloat16, dy.numel());
    TORCH_CHECK(s.sizes() == dy.sizes(), "layernorm_backward: s must match dy");
    const int D = narrow(dy.size(-1), op, "the row length");
    TORCH_CHECK(kfk::layernorm_supported(D), "layernorm_backward: unsupported row length ", D);
    const int64_t rows = dy.numel() / D;
    check_dense(gamma, op, "gamma", dev, at::kFloat, D);
    check_dense(mean, op, "mean", dev, at::kFloat, rows);
    check_dense(rstd, op, "rstd", dev, at::kFloat, rows);
    const bool rb = rbias_dtype.has_value();
    TORCH_CHECK(!rb || *rbias_dtype == at::kFloat || *rbias_dtype == at::kBFloat16,
                "layernorm_backward: rbias_dtype must be float32 or bfloat16");
    c10::DeviceGuard gd(dy.device());
    auto ds = at::empty_like(dy);
    auto partial = at::empty({kfk::layernorm_bwd_blocks(rows), rb ? 3 : 2, D}, dy.options().dtype(at::kFloat));
    at::Tensor rbias;
    SumOut ro{nullptr, nullptr};
    if (rb) {
        rbias = at::empty({D}, dy.options().dtype(*rbias_dtype));
        ro = sum_out(rbias);
    }
    auto dgamma = at::empty({D}, dy.options().dtype(at::kFloat));
    auto dbeta = at::empty({D}, dy.options().dtype(at::kFloat));
    at::Tensor dr;
    if (p > 0) dr = at::empty_like(dy);
    kfk::launch_layernorm_backward(bf16(dy), bf16(s), gamma.data_ptr<float>(), mean.data_ptr<float>(),
                                   rstd.data_ptr<float>(), bf16_mut(ds), partial.data_ptr<float>(),
                                   dgamma.data_ptr<float>(), dbeta.data_ptr<float>(), rows, D, stream_of(dy, 0),
                                   dr.defined() ? bf16_mut(dr) : nullptr, static_cast<float>(p),
                                   static_cast<uint32_t>(seed), ro.f32, ro.b16);
    if (rb) return {ds, dgamma, dbeta, dr, rbias};
    return {ds, dgamma, dbeta, dr};
}

// The operands of gemm.hip's a[M, K] . b[N, K]^T (+ bias): returns {M, N, K} and the bias pointer (or null).
struct NT {
    int64_t M, N, K;
    const uint16_t *bias;
};
NT check_nt(const char *op, const at::Tensor &a, const at::Tensor &b, const OptTensor &bias) {
    TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && a.size(1) == b.size(1), op, ": a must be [M, K] and b [N, K]");
    check_dense(a, op, "a", kAnyGpu, at::kBFloat16, a.numel());
    check_dense(b, op, "b", a.device(), at::kBFloat16, b.numel());
    NT r{a.size(0), b.size(0), a.size(1), nullptr};
    if (has(bias)) {
        check_dense(*bias, op, "bias", a.device(), at::kBFloat16, r.N);
        r.bias = bf16(*bias);
    }
    return r;
}

// gemm.hip: out[M, N] = a[M, K] . b[N, K]^T (+ bias) (+ out when accumulate), bf16.
// C[M, ldc] (only columns < N written, the chunk holding column N - 1 whole) = a . b^T (+ bias), for a
// ragged N (BERT's 30,522-entry vocabulary): rows of C padded to ldc (a multiple of 8) stay 16-byte aligned
at::Tensor gemm_nt_ld(at::Tensor a, at::Tensor b, OptTensor bias, int64_t ldc, int64_t bn) {
    const char *op = "gemm_nt_ld";
    const auto [M, N, K, bp] = check_nt(op, a, b, bias);
    if (ldc <= 0) ldc = (N + 7) / 8 * 8;
    TORCH_CHECK(kfk::gemm_nt_ld_supported(M, N, K, ldc), "gemm_nt_ld: unsupported shape M=", M, " N=", N, " K=", K,
                " ldc=", ldc);
    const int tile = bn > 0 ? narrow(bn, op, "bn") : 256;
    c10::DeviceGuard gd(a.device());
    auto c = at::empty({M, ldc}, a.options());
    kfk::launch_gemm_nt_ld(bf16(a), bf16(b), bf16_mut(c), bp, narrow(M, op, "M"), narrow(N, op, "N"), narrow(K, op, "K"),
                           narrow(ldc, op, "ldc"), bp ? kfk::kGemmBias : 0, tile, stream_of(a, 0));
    return c;
}

at::Tensor gemm_nt(at::Tensor a, at::Tensor b, OptTensor bias, OptTensor out, bool accumulate, int64_t bn) {
    const char *op = "gemm_nt";
    const auto [M, N, K, bp] = check_nt(op, a, b, bias);
    TORCH_CHECK(kfk::gemm_nt_supported(M, N, K), "gemm_nt: unsupported shape M=", M, " N=", N, " K=", K);
    TORCH_CHECK(has(out) || !accumulate, "gemm_nt: accumulate needs out");
    int epi = bp ? kfk::kGemmBias : 0;
    if (accumulate) epi |= kfk::kGemmAccum;
    const int tile = narrow(bn, op, "bn");
    c10::DeviceGuard gd(a.device());
    auto c = out_or_empty(out, {M, N}, a.options(), op).first;
    kfk::launch_gemm_nt(bf16(a), bf16(b), bf16_mut(c), bp, narrow(M, op, "M"), narrow(N, op, "N"), narrow(K, op, "K"),
                        epi, tile, stream_of(a, 0));
    return c;
}

// gemm.hip GELU-gradient epilogue: (du [M, N] bf16, db [N]) with du = bf16(bf16(a . b^T) * gelu'(u)) and
// db the column sums of du (f32 or bf16 as bias_dtype) -- the data gradient through GELU of the layer
// whose output u (its pre-activation) fed gelu, and that layer's bias gradient, in one GEMM + fold.
std::vector<at::Tensor> gemm_nt_gelu_grad(at::Tensor a, at::Tensor b, at::Tensor u,
                                          c10::optional<at::ScalarType> bias_dtype) {
    const char *op = "gemm_nt_gelu_grad";
    const auto [M, N, K, bp] = check_nt(op, a, b, OptTensor());
    check_dense(u, op, "u", a.device(), at::kBFloat16, M * N);
    TORCH_CHECK(kfk::gemm_nt_supported(M, N, K) && N % 256 == 0, "gemm_nt_gelu_grad: unsupported shape M=", M, " N=", N,
                " K=", K);
    const int m = narrow(M, op, "M"), n = narrow(N, op, "N"), k = narrow(K, op, "K");
    c10::DeviceGuard gd(a.device());
    auto c = at::empty({M, N}, a.options());
    const int rows = kfk::gemm_nt_gelu_grad_rows(m);
    auto part = at::empty({rows, N}, a.options().dtype(at::kFloat));
    const bool f32 = !bias_dtype || *bias_dtype == at::kFloat;
    auto db = at::empty({N}, a.options().dtype(f32 ? at::kFloat : at::kBFloat16));
    const auto so = sum_out(db);
    const auto s = stream_of(a, 0);
    kfk::launch_gemm_nt_gelu_grad(bf16(a), bf16(b), bf16_mut(c), bf16(u), part.data_ptr<float>(), m, n, k, s);
    kfk::launch_colsum_fold(part.data_ptr<float>(), rows, n, so.f32, so.b16, s);
    return {c, db};
}

}  // namespace

void bind_bert(py::module_ &m) {
    m.def("xent_forward", &xent_forward, "fused softmax cross-entropy over bf16 logits: (lse, per-row loss)");
    m.def("xent_backward", &xent_backward, "its bf16 logit gradient, scaled by scale[0]");
    m.def("gelu_backward_colsum", &gelu_backward_colsum, "erf-GELU backward du and the column sums of du",
          py::arg("dy"), py::arg("u"), py::arg("dtype"));
    m.def("colsum", &colsum, "column sums of a bf16 [T, O] matrix (bias gradient), deterministic", py::arg("x"),
          py::arg("dtype"));
    m.def("layernorm_supported", &kfk::layernorm_supported);
    m.def("layernorm_forward", &layernorm_forward, "fused residual-add + LayerNorm (bf16 rows) -> (y, s, mean, rstd)",
          py::arg("x"), py::arg("r"), py::arg("gamma"), py::arg("beta"), py::arg("eps"), py::arg("p") = 0.0,
          py::arg("seed") = 0);
    m.def("layernorm_backward", &layernorm_backward,
          "LayerNorm backward -> (ds, dgamma, dbeta, dr or None[, residual-input bias gradient])", py::arg("dy"),
          py::arg("s"), py::arg("gamma"), py::arg("mean"), py::arg("rstd"), py::arg("p") = 0.0, py::arg("seed") = 0,
          py::arg("rbias_dtype") = py::none());
    m.def("attention_supported", &kfk::attention_supported);
    m.def("attention_forward", &attention_forward,
          "fused self-attention forward (S 64..512 in steps of 64, head dim 64, dropout) -> (out, lse); "
          "stream_kernel: S = 128 on the streaming kernels that serve S > 128",
          py::arg("qkv"), py::arg("heads"), py::arg("scale"), py::arg("seed"), py::arg("p_drop"),
          py::arg("stream_kernel") = false);
    m.def("attention_backward", &attention_backward, "fused self-attention backward -> dqkv (S as the forward)",
          py::arg("qkv"), py::arg("out"), py::arg("lse"), py::arg("dout"), py::arg("heads"), py::arg("scale"),
          py::arg("seed"), py::arg("p_drop"), py::arg("stream_kernel") = false);
    m.def("gemm_nt", &gemm_nt, py::arg("a"), py::arg("b"), py::arg("bias") = py::none(), py::arg("out") = py::none(),
          py::arg("accumulate") = false, py::arg("bn") = -1,
          "bf16 a[M,K] . b[N,K]^T (+bias) (+out) on the pipelined 256 x bn MFMA GEMM (gemm.hip)");
    m.def("gemm_nt_supported", &kfk::gemm_nt_supported);
    m.def("gemm_nt_ld", &gemm_nt_ld, py::arg("a"), py::arg("b"), py::arg("bias") = py::none(), py::arg("ldc") = 0,
          py::arg("bn") = 256, "C [M, ldc] = a . b^T (+ bias) for any N (columns >= N of C unspecified)");
    m.def("gemm_nt_ld_supported", &kfk::gemm_nt_ld_supported);
    m.def("gemm_nt_gelu_grad", &gemm_nt_gelu_grad, "(du, db): the GELU backward fused into the data-gradient NT GEMM "
          "(du = bf16(bf16(a . b^T) * gelu'(u)), db = column sums of du)", py::arg("a"), py::arg("b"), py::arg("u"),
          py::arg("bias_dtype") = py::none());
    m.def("gemm_nt_pick_bn", &kfk::gemm_nt_pick_bn);
    m.def(
        "set_dropout_seed_base",
        [](OptTensor t) {
            if (!has(t)) {
                kfk::set_dropout_seed_base(nullptr);
                return;
            }
            check_dense(*t, "set_dropout_seed_base", "base", kAnyGpu, at::kInt, 1, true);
            kfk::set_dropout_seed_base(reinterpret_cast<const uint32_t *>(t->data_ptr()));
        },
        py::arg("base"), "device word mixed into every hashed dropout seed (None: host seeds only)");
}
