// Flat-buffer ops: reduce, optimizer steps, casts, norms, pack / unpack, gradient accumulation.
#include "bind_util.hpp"

#include <vector>

using namespace kfb;

namespace {

void reduce_op(at::Tensor z, at::Tensor x, at::Tensor y, int64_t op) {
    check_gpu(z, "z");
    check_gpu(x, "x");
    check_gpu(y, "y");
    TORCH_CHECK(x.numel() == y.numel() && z.numel() == x.numel(), "reduce: size mismatch");
    TORCH_CHECK(x.scalar_type() == y.scalar_type() && z.scalar_type() == x.scalar_type(), "reduce: dtype mismatch");
    c10::DeviceGuard g(z.device());
    kfk::launch_reduce(z.data_ptr(), x.data_ptr(), y.data_ptr(), x.numel(), dtype_code(x), narrow(op, "reduce", "op"),
                       stream_of(z, 0));
}

void sgd_step(at::Tensor w, at::Tensor g, OptTensor m, OptTensor shadow, double lr, OptTensor lr_t, double mu,
              double damp, double wd, double gscale, bool nesterov, bool first) {
    check_gpu(w, "w");
    check_gpu(g, "g");
    TORCH_CHECK(w.scalar_type() == at::kFloat && g.scalar_type() == at::kFloat, "sgd_step: f32 buffers required");
    TORCH_CHECK(w.numel() == g.numel(), "sgd_step: size mismatch");
    float *mp = nullptr;
    if (has(m)) {
        check_gpu(*m, "m");
        TORCH_CHECK(m->numel() == w.numel() && m->scalar_type() == at::kFloat, "sgd_step: bad momentum buffer");
        mp = m->data_ptr<float>();
    }
    uint16_t *sp = nullptr;
    if (has(shadow)) {
        TORCH_CHECK(shadow->scalar_type() == at::kBFloat16 && shadow->numel() == w.numel(), "sgd_step: bad shadow");
        sp = bf16_mut(*shadow);
    }
    const float *lrp = nullptr;
    if (has(lr_t)) {
        TORCH_CHECK(lr_t->is_cuda() && lr_t->scalar_type() == at::kFloat, "sgd_step: lr tensor must be f32 on GPU");
        lrp = lr_t->data_ptr<float>();
    }
    c10::DeviceGuard gd(w.device());
    kfk::launch_sgd(w.data_ptr<float>(), g.data_ptr<float>(), mp, sp, w.numel(), static_cast<float>(lr), lrp,
                    static_cast<float>(mu), static_cast<float>(damp), static_cast<float>(wd),
                    static_cast<float>(gscale), nesterov, first, stream_of(w, 0));
}

void adam_step(at::Tensor w, at::Tensor g, at::Tensor m, at::Tensor v, double lr, OptTensor lr_t, double b1, double b2,
               double eps, double wd, bool adamw, double gscale, at::Tensor step, OptTensor shadow) {
    for (auto *t : {&w, &g, &m, &v}) {
        check_gpu(*t, "adam buffer");
        TORCH_CHECK(t->scalar_type() == at::kFloat && t->numel() == w.numel(), "adam_step: f32 buffers of equal size");
    }
    TORCH_CHECK(step.is_cuda() && step.scalar_type() == at::kFloat, "adam_step: step must be an f32 GPU tensor");
    const float *lrp = has(lr_t) ? lr_t->data_ptr<float>() : nullptr;
    uint16_t *sh = nullptr;
    if (has(shadow)) {
        check_dense(*shadow, "adam_step", "shadow", w.device(), at::kBFloat16, w.numel());
        sh = bf16_mut(*shadow);
    }
    c10::DeviceGuard gd(w.device());
    kfk::launch_adam(w.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(), w.numel(),
                     static_cast<float>(lr), lrp, static_cast<float>(b1), static_cast<float>(b2),
                     static_cast<float>(eps), static_cast<float>(wd), adamw, static_cast<float>(gscale),
                     step.data_ptr<float>(), stream_of(w, 0), sh);
}

// The slot / chunk tables of lars_step and lamb_step.  offsets is a host int64 tensor of nseg + 1 slot
// starts (read here, on every call: a few hundred words); everything else lives on w's device.
kfk::LayerTables layer_tables(const char *op, const at::Tensor &w, const at::Tensor &offsets, const at::Tensor &chunks,
                              const at::Tensor &slot_chunk0, const at::Tensor &partials, const at::Tensor &wd_tab,
                              const at::Tensor &trust_tab, const at::Tensor &w_norm, const at::Tensor &x_norm,
                              const at::Tensor &ratio) {
    TORCH_CHECK(offsets.device().is_cpu() && offsets.scalar_type() == at::kLong && offsets.dim() == 1 &&
                    offsets.is_contiguous() && offsets.numel() >= 2,
                op, ": offsets must be a host int64 vector of nseg + 1 slot starts");
    const int64_t *off = offsets.data_ptr<int64_t>();
    const int64_t nseg = offsets.numel() - 1;
    TORCH_CHECK(off[0] == 0 && off[nseg] == w.numel(), op, ": offsets must start at 0 and end at numel (", w.numel(),
                ")");
    int64_t nchunks = 0;
    for (int64_t k = 0; k < nseg; ++k) {
        TORCH_CHECK(off[k + 1] > off[k], op, ": offsets must be ascending (slot ", k, ")");
        TORCH_CHECK(off[k + 1] % 64 == 0, op, ": offsets must be multiples of 64 (slot ", k + 1, ")");
        nchunks += (off[k + 1] - off[k] + kfk::kLayerChunk - 1) / kfk::kLayerChunk;
    }
    const Dev dev = w.device();
    TORCH_CHECK(chunks.dim() == 2 && chunks.size(1) == 3, op, ": chunks must be an int64 [", nchunks, ", 3] tensor");
    check_dense(chunks, op, "chunks", dev, at::kLong, 3 * nchunks);
    check_dense(slot_chunk0, op, "slot_chunk0", dev, at::kLong, nseg + 1);
    check_dense(partials, op, "partials", dev, at::kFloat, 2 * nchunks);
    check_dense(wd_tab, op, "wd_tab", dev, at::kFloat, nseg);
    check_dense(trust_tab, op, "trust_tab", dev, at::kFloat, nseg);
    check_dense(w_norm, op, "w_norm", dev, at::kFloat, nseg);
    check_dense(x_norm, op, "x_norm", dev, at::kFloat, nseg);
    check_dense(ratio, op, "ratio", dev, at::kFloat, nseg);
    kfk::LayerTables t;
    t.chunks = chunks.data_ptr<int64_t>();
    t.slot_chunk0 = slot_chunk0.data_ptr<int64_t>();
    t.nchunks = narrow(nchunks, op, "the chunk count");
    t.nseg = narrow(nseg, op, "the slot count");
    t.partials = partials.data_ptr<float>();
    t.wd_tab = wd_tab.data_ptr<float>();
    t.trust_tab = trust_tab.data_ptr<float>();
    t.w_norm = w_norm.data_ptr<float>();
    t.x_norm = x_norm.data_ptr<float>();
    t.ratio = ratio.data_ptr<float>();
    return t;
}

// the layer-wise kernels move float4s: a view that starts inside a 16-byte word is refused
void check_flat_f32(const at::Tensor &t, const char *op, const char *name, const at::Tensor &w) {
    check_dense(t, op, name, w.device(), at::kFloat, w.numel());
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, op, ": ", name, " must be 16-byte aligned");
}

const float *lr_ptr(const char *op, const OptTensor &lr_t, const Dev &dev) {
    if (!has(lr_t)) return nullptr;
    check_dense(*lr_t, op, "lr_t", dev, at::kFloat, 1);
    return lr_t->data_ptr<float>();
}

uint16_t *shadow_ptr(const char *op, const OptTensor &shadow, const at::Tensor &w) {
    if (!has(shadow)) return nullptr;
    check_dense(*shadow, op, "shadow", w.device(), at::kBFloat16, w.numel());
    TORCH_CHECK(reinterpret_cast<uintptr_t>(shadow->data_ptr()) % 8 == 0, op, ": shadow must be 8-byte aligned");
    return bf16_mut(*shadow);
}

void lars_step(at::Tensor w, at::Tensor g, OptTensor m, OptTensor shadow, at::Tensor offsets, at::Tensor chunks,
               at::Tensor slot_chunk0, at::Tensor partials, at::Tensor wd_tab, at::Tensor trust_tab, at::Tensor w_norm,
               at::Tensor x_norm, at::Tensor ratio, double lr, OptTensor lr_t, double mu, double tc, double eps,
               double gscale, bool nesterov) {
    const char *op = "lars_step";
    check_gpu(w, "lars_step: w");
    check_flat_f32(w, op, "w", w);
    check_flat_f32(g, op, "g", w);
    float *mp = nullptr;
    if (has(m)) {
        check_flat_f32(*m, op, "m", w);
        mp = m->data_ptr<float>();
    }
    TORCH_CHECK(mu == 0.0 || mp, op, ": m must be given with a momentum");
    uint16_t *sp = shadow_ptr(op, shadow, w);
    const float *lrp = lr_ptr(op, lr_t, w.device());
    const auto t = layer_tables(op, w, offsets, chunks, slot_chunk0, partials, wd_tab, trust_tab, w_norm, x_norm, ratio);
    c10::DeviceGuard gd(w.device());
    kfk::launch_lars(w.data_ptr<float>(), g.data_ptr<float>(), mp, sp, w.numel(), t, static_cast<float>(lr), lrp,
                     static_cast<float>(mu), static_cast<float>(tc), static_cast<float>(eps),
                     static_cast<float>(gscale), nesterov, stream_of(w, 0));
}

// max_grad_norm <= 0: no clipping; else gnorm_ws (f32, 2 * grid cap + 2 words) is the scratch of the
// sum-of-squares pass over g that runs ahead of the partial-norm stage.
void lamb_step(at::Tensor w, at::Tensor g, at::Tensor m, at::Tensor v, OptTensor shadow, at::Tensor offsets,
               at::Tensor chunks, at::Tensor slot_chunk0, at::Tensor partials, at::Tensor wd_tab, at::Tensor trust_tab,
               at::Tensor w_norm, at::Tensor x_norm, at::Tensor ratio, double lr, OptTensor lr_t, double b1, double b2,
               double eps, double gscale, at::Tensor step, bool bias_correction, double max_grad_norm,
               OptTensor gnorm_ws) {
    const char *op = "lamb_step";
    check_gpu(w, "lamb_step: w");
    check_flat_f32(w, op, "w", w);
    check_flat_f32(g, op, "g", w);
    check_flat_f32(m, op, "m", w);
    check_flat_f32(v, op, "v", w);
    check_dense(step, op, "step", w.device(), at::kFloat, 1);
    uint16_t *sp = shadow_ptr(op, shadow, w);
    const float *lrp = lr_ptr(op, lr_t, w.device());
    const auto t = layer_tables(op, w, offsets, chunks, slot_chunk0, partials, wd_tab, trust_tab, w_norm, x_norm, ratio);
    float *ws = nullptr;
    if (max_grad_norm > 0.0) {
        TORCH_CHECK(has(gnorm_ws), op, ": gnorm_ws must be given with max_grad_norm");
        check_dense(*gnorm_ws, op, "gnorm_ws", w.device(), at::kFloat, 2 * kfk::kMaxGridHost + 2);
        ws = gnorm_ws->data_ptr<float>();
    }
    c10::DeviceGuard gd(w.device());
    auto s = stream_of(w, 0);
    const float *gsq = nullptr;
    if (ws) {
        float *out = ws + 2 * kfk::kMaxGridHost;
        kfk::launch_sumsq2(g.data_ptr<float>(), nullptr, w.numel(), dtype_code(g), ws, out, s);
        gsq = out;
    }
    kfk::launch_lamb(w.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(), sp, w.numel(),
                     t, static_cast<float>(lr), lrp, b1, b2, static_cast<float>(eps), static_cast<float>(gscale),
                     step.data_ptr<float>(), bias_correction, static_cast<float>(max_grad_norm), gsq, s);
}

void axpby(at::Tensor y, at::Tensor x, OptTensor z, double a, double b) {
    check_gpu(y, "y");
    check_gpu(x, "x");
    TORCH_CHECK(x.numel() == y.numel() && x.scalar_type() == y.scalar_type(), "axpby: mismatch");
    TORCH_CHECK(y.scalar_type() == at::kFloat || y.scalar_type() == at::kBFloat16, "axpby: f32/bf16 only");
    void *zp = nullptr;
    if (has(z)) {
        check_gpu(*z, "z");
        TORCH_CHECK(z->numel() == y.numel() && z->scalar_type() == y.scalar_type(), "axpby: bad z");
        zp = z->data_ptr();
    }
    c10::DeviceGuard gd(y.device());
    kfk::launch_axpby(y.data_ptr(), x.data_ptr(), zp, y.numel(), static_cast<float>(a), static_cast<float>(b),
                      dtype_code(y), stream_of(y, 0));
}

void scale_(at::Tensor x, double alpha) {
    check_gpu(x, "x");
    int dt = dtype_code(x);
    TORCH_CHECK(dt == 8 || dt == 9 || dt == 10, "scale_: float types only");
    c10::DeviceGuard gd(x.device());
    kfk::launch_scale(x.data_ptr(), x.numel(), static_cast<float>(alpha), dt, stream_of(x, 0));
}

void square(at::Tensor dst, at::Tensor src) {
    check_gpu(dst, "dst");
    check_gpu(src, "src");
    TORCH_CHECK(dst.scalar_type() == at::kFloat && dst.numel() == src.numel(), "square: f32 dst of equal size");
    c10::DeviceGuard gd(dst.device());
    kfk::launch_square(dst.data_ptr<float>(), src.data_ptr(), src.numel(), dtype_code(src), stream_of(dst, 0));
}

void cast_copy(at::Tensor dst, at::Tensor src, double scale) {
    check_gpu(dst, "dst");
    check_gpu(src, "src");
    const int sd = dtype_code(src), dd = dtype_code(dst);
    TORCH_CHECK((sd == 9 || sd == 10) && (dd == 9 || dd == 10), "cast_copy: f32/bf16 only");
    TORCH_CHECK(dst.numel() == src.numel() && dst.device() == src.device(), "cast_copy: size/device mismatch");
    c10::DeviceGuard gd(dst.device());
    kfk::launch_cast(dst.data_ptr(), src.data_ptr(), src.numel(), sd, dd, static_cast<float>(scale), stream_of(dst, 0));
}

at::Tensor sumsq2(at::Tensor a, OptTensor b) {
    check_gpu(a, "a");
    int dt = dtype_code(a);
    TORCH_CHECK(dt == 9 || dt == 10, "sumsq2: f32/bf16 only");
    const void *bp = nullptr;
    if (has(b)) {
        check_gpu(*b, "b");
        TORCH_CHECK(b->numel() == a.numel() && b->scalar_type() == a.scalar_type(), "sumsq2: mismatch");
        bp = b->data_ptr();
    }
    c10::DeviceGuard gd(a.device());
    auto opts = a.options().dtype(at::kFloat);
    auto partials = at::empty({2 * kfk::kMaxGridHost}, opts);
    auto out = at::empty({2}, opts);
    kfk::launch_sumsq2(a.data_ptr(), bp, a.numel(), dt, partials.data_ptr<float>(), out.data_ptr<float>(),
                       stream_of(a, 0));
    return out;
}

at::Tensor variance(at::Tensor s1, at::Tensor s2, double inv_np) {
    check_gpu(s1, "s1");
    check_gpu(s2, "s2");
    TORCH_CHECK(s1.scalar_type() == at::kFloat && s2.scalar_type() == at::kFloat && s1.numel() == s2.numel(),
                "variance: f32 buffers of equal size");
    c10::DeviceGuard gd(s1.device());
    auto opts = s1.options();
    auto partials = at::empty({kfk::kMaxGridHost}, opts);
    auto out = at::empty({1}, opts);
    kfk::launch_variance(s1.data_ptr<float>(), s2.data_ptr<float>(), s1.numel(), static_cast<float>(inv_np),
                         partials.data_ptr<float>(), out.data_ptr<float>(), stream_of(s1, 0));
    return out;
}

// Per-tensor L2 norms of E[g^2]-E[g]^2 summed over tensors (the reference's
// gradient variance, grad_variance.py:46-59).  seg_off: int64 GPU [nseg+1].
at::Tensor seg_variance(at::Tensor s1, at::Tensor s2, at::Tensor seg_off, double inv_np) {
    check_gpu(s1, "s1");
    check_gpu(s2, "s2");
    TORCH_CHECK(seg_off.is_cuda() && seg_off.scalar_type() == at::kLong && seg_off.numel() >= 2,
                "seg_variance: int64 GPU offsets required");
    TORCH_CHECK(s1.scalar_type() == at::kFloat && s2.scalar_type() == at::kFloat && s1.numel() == s2.numel(),
                "seg_variance: f32 buffers of equal size");
    c10::DeviceGuard gd(s1.device());
    const int nseg = narrow(seg_off.numel() - 1, "seg_variance", "the segment count");
    auto out = at::zeros({nseg}, s1.options());
    kfk::launch_seg_variance(s1.data_ptr<float>(), s2.data_ptr<float>(), s1.numel(), static_cast<float>(inv_np),
                             seg_off.data_ptr<int64_t>(), nseg, out.data_ptr<float>(), stream_of(s1, 0));
    return out.sqrt().sum();
}

void gns_update(at::Tensor sumsq_small, at::Tensor sumsq_big, double b_small, double b_big, double alpha,
                at::Tensor state) {
    TORCH_CHECK(state.is_cuda() && state.scalar_type() == at::kFloat && state.numel() >= 4, "gns_update: bad state");
    c10::DeviceGuard gd(state.device());
    kfk::launch_gns_update(sumsq_small.data_ptr<float>(), sumsq_big.data_ptr<float>(), static_cast<float>(b_small),
                           static_cast<float>(b_big), static_cast<float>(alpha), state.data_ptr<float>(),
                           stream_of(state, 0));
}

// desc: int64 GPU tensor [n, 3] of (ptr, offset, numel), sorted by offset.
void pack(at::Tensor desc, int64_t n_tensors, int64_t src_dtype, at::Tensor flat, double scale) {
    check_gpu(flat, "flat");
    TORCH_CHECK(desc.is_cuda() && desc.scalar_type() == at::kLong, "pack: desc must be int64 on GPU");
    c10::DeviceGuard gd(flat.device());
    kfk::launch_pack(desc.data_ptr<int64_t>(), narrow(n_tensors, "pack", "n_tensors"), flat.numel(), flat.data_ptr(),
                     dtype_code(flat), narrow(src_dtype, "pack", "src_dtype"), static_cast<float>(scale),
                     stream_of(flat, 0));
}

void unpack(at::Tensor desc, int64_t n_tensors, int64_t dst_dtype, at::Tensor flat, double scale) {
    check_gpu(flat, "flat");
    TORCH_CHECK(desc.is_cuda() && desc.scalar_type() == at::kLong, "unpack: desc must be int64 on GPU");
    c10::DeviceGuard gd(flat.device());
    kfk::launch_unpack(desc.data_ptr<int64_t>(), narrow(n_tensors, "unpack", "n_tensors"), flat.numel(),
                       flat.data_ptr(), dtype_code(flat), narrow(dst_dtype, "unpack", "dst_dtype"),
                       static_cast<float>(scale), stream_of(flat, 0));
}

// flat[offsets[i] : offsets[i] + srcs[i].numel()] += scale * srcs[i] (memory order), batched into
// launches of up to GradAccTable::kMax same-dtype tensors.  srcs must be dense (any stride
// permutation); the caller guarantees the flat slot uses the same memory order.
void grad_accumulate(at::Tensor flat, std::vector<at::Tensor> srcs, std::vector<int64_t> offsets, double scale) {
    check_gpu(flat, "flat");
    TORCH_CHECK(flat.scalar_type() == at::kFloat && flat.is_contiguous(), "grad_accumulate: flat must be f32");
    TORCH_CHECK(srcs.size() == offsets.size(), "grad_accumulate: srcs/offsets length mismatch");
    for (const auto &t : srcs)
        TORCH_CHECK(dtype_code(t) == 9 || dtype_code(t) == 10,
                    "grad_accumulate: bf16 or f32 sources only");
    // Sources are consumed on the current stream, the one they were produced
    // on, so the caching allocator's stream-ordered reuse keeps them valid.
    c10::DeviceGuard gd(flat.device());
    auto s = stream_of(flat, 0);
    for (int dt : {9, 10}) {
        kfk::GradAccTable tab;
        tab.src_dtype = dt;
        tab.scale = static_cast<float>(scale);
        tab.blk_start[0] = 0;
        auto flush = [&] {
            kfk::launch_grad_accumulate(tab, flat.data_ptr<float>(), s);
            tab.n = 0;
        };
        for (size_t i = 0; i < srcs.size(); ++i) {
            const auto &t = srcs[i];
            if (dtype_code(t) != dt) continue;
            TORCH_CHECK(t.device() == flat.device(), "grad_accumulate: device mismatch");
            TORCH_CHECK(t.is_non_overlapping_and_dense(), "grad_accumulate: source must be dense");
            TORCH_CHECK(offsets[i] >= 0 && offsets[i] + t.numel() <= flat.numel(), "grad_accumulate: out of range");
            if (t.numel() == 0) continue;
            const int k = tab.n;
            tab.src[k] = t.data_ptr();
            tab.off[k] = offsets[i];
            tab.numel[k] = t.numel();
            tab.blk_start[k + 1] = tab.blk_start[k] + kfk::grad_accumulate_blocks(t.numel());
            tab.n = k + 1;
            if (tab.n == kfk::GradAccTable::kMax) flush();
        }
        flush();
    }
}

// grad[V, D] (f32, accumulated into) += scatter of dy[T, D] (f32 / bf16) by ids[T] (int64)
void embedding_backward(at::Tensor grad, at::Tensor ids, at::Tensor dy, int64_t ch) {
    check_gpu(grad, "grad");
    check_gpu(ids, "ids");
    check_gpu(dy, "dy");
    TORCH_CHECK(grad.scalar_type() == at::kFloat && grad.dim() == 2, "embedding_backward: grad f32 [V, D]");
    TORCH_CHECK(ids.scalar_type() == at::kLong, "embedding_backward: ids int64");
    const int64_t V = grad.size(0), D = grad.size(1), T = ids.numel();
    TORCH_CHECK(dy.numel() == T * D && (dy.scalar_type() == at::kFloat || dy.scalar_type() == at::kBFloat16),
                "embedding_backward: dy f32/bf16 [T, D]");
    TORCH_CHECK(D % 4 == 0, "embedding_backward: D % 4");
    c10::DeviceGuard gd(grad.device());
    kfk::launch_embedding_backward(grad.data_ptr<float>(), ids.data_ptr<int64_t>(), dy.data_ptr(),
                                   dy.scalar_type() == at::kBFloat16, T, narrow(D, "embedding_backward", "D"), V,
                                   stream_of(grad, 0), narrow(ch, "embedding_backward", "ch"));
}

}  // namespace

void bind_flat(py::module_ &m) {
    m.def("reduce", &reduce_op, "K1: z = op(x, y)");
    m.def("sgd_step", &sgd_step, "K8: fused SGD/momentum/nesterov/wd step on flat f32 buffers", py::arg("w"),
          py::arg("g"), py::arg("m"), py::arg("shadow"), py::arg("lr"), py::arg("lr_t"), py::arg("mu"),
          py::arg("damp"), py::arg("wd"), py::arg("gscale"), py::arg("nesterov"), py::arg("first"));
    m.def("adam_step", &adam_step, "fused Adam/AdamW step on flat f32 buffers (shadow: also bf16(w) there)",
          py::arg("w"), py::arg("g"), py::arg("m"), py::arg("v"), py::arg("lr"), py::arg("lr_t"), py::arg("b1"),
          py::arg("b2"), py::arg("eps"), py::arg("wd"), py::arg("adamw"), py::arg("gscale"), py::arg("step"),
          py::arg("shadow") = py::none());
    m.def("lars_step", &lars_step, "fused LARS step on a flat f32 space: per-slot norms, trust ratio, apply",
          py::arg("w"), py::arg("g"), py::arg("m"), py::arg("shadow"), py::arg("offsets"), py::arg("chunks"),
          py::arg("slot_chunk0"), py::arg("partials"), py::arg("wd_tab"), py::arg("trust_tab"), py::arg("w_norm"),
          py::arg("x_norm"), py::arg("ratio"), py::arg("lr"), py::arg("lr_t"), py::arg("mu"), py::arg("tc"),
          py::arg("eps"), py::arg("gscale"), py::arg("nesterov"));
    m.def("lamb_step", &lamb_step, "fused LAMB step on a flat f32 space: moments + per-slot norms, trust ratio, apply",
          py::arg("w"), py::arg("g"), py::arg("m"), py::arg("v"), py::arg("shadow"), py::arg("offsets"),
          py::arg("chunks"), py::arg("slot_chunk0"), py::arg("partials"), py::arg("wd_tab"), py::arg("trust_tab"),
          py::arg("w_norm"), py::arg("x_norm"), py::arg("ratio"), py::arg("lr"), py::arg("lr_t"), py::arg("b1"),
          py::arg("b2"), py::arg("eps"), py::arg("gscale"), py::arg("step"), py::arg("bias_correction"),
          py::arg("max_grad_norm") = 0.0, py::arg("gnorm_ws") = py::none());
    // elements per chunk of the layer-wise kernels and the cap of their chunk-loop grid
    m.attr("layerwise_chunk") = kfk::kLayerChunk;
    m.attr("layerwise_grid_cap") = kfk::kLayerGridCap;
    m.def("axpby", &axpby, "y = a*y + b*x (optionally also z = y)", py::arg("y"), py::arg("x"), py::arg("z"),
          py::arg("a"), py::arg("b"));
    m.def("scale_", &scale_, "x *= alpha");
    m.def("square", &square, "dst = src^2");
    m.def("cast_copy", &cast_copy, "dst = scale * src with an f32 <-> bf16 cast");
    m.def("sumsq2", &sumsq2, "[sum(a^2), sum(b^2)] in one pass", py::arg("a"), py::arg("b") = py::none());
    m.def("variance", &variance, "sum |s2*inv - (s1*inv)^2|");
    m.def("gns_update", &gns_update, "device-side gradient-noise-scale EMA update");
    m.def("seg_variance", &seg_variance, "sum_k ||E[g^2]-E[g]^2||_2 over flat tensor segments");
    m.def("grad_accumulate", &grad_accumulate, "flat[off_i:] += scale * src_i for a list of bf16/f32 tensors",
          py::arg("flat"), py::arg("srcs"), py::arg("offsets"), py::arg("scale") = 1.0);
    m.def("pack", &pack, "multi-tensor pack into a flat buffer");
    m.def("unpack", &unpack, "multi-tensor unpack from a flat buffer");
    m.def("embedding_backward", &embedding_backward, py::arg("grad"), py::arg("ids"), py::arg("dy"), py::arg("ch") = 0,
          "grad[ids[t]] += dy[t] by f32 atomics (graph-replayable embedding gradient)");
}
