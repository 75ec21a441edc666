// Argument checks shared by the kungfu_amd._hip bindings (bind_*.cpp).
//
// Every refusal reads "<op>: <argument> must be ...": it begins with the binding's Python name and
// names the argument.  `dev` is the device an operand has to live on; the leading tensor of a
// binding passes kAnyGpu and only has to be on some GPU.  All of these run on the host before
// anything is allocated or launched.
#pragma once

#include <ATen/hip/HIPContext.h>
#include <c10/core/DeviceGuard.h>
#include <torch/extension.h>

#include "kernels.hpp"

#include <climits>
#include <initializer_list>
#include <utility>

namespace kfb {

using OptTensor = c10::optional<at::Tensor>;
using Dev = c10::optional<at::Device>;
inline const Dev kAnyGpu{};

inline int dtype_code(const at::Tensor &t) {
    switch (t.scalar_type()) {
    case at::kByte: return 0;
    case at::kChar: return 4;
    case at::kInt: return 6;
    case at::kLong: return 7;
    case at::kHalf: return 8;
    case at::kBFloat16: return 9;
    case at::kFloat: return 10;
    case at::kDouble: return 11;
    case at::kBool: return 12;
    default: TORCH_CHECK(false, "kungfu_amd._hip: unsupported dtype ", t.scalar_type());
    }
    return -1;
}

inline hipStream_t stream_of(const at::Tensor &t, int64_t stream) {
    if (stream) return reinterpret_cast<hipStream_t>(stream);
    return c10::hip::getCurrentHIPStream(t.device().index()).stream();
}

inline void check_gpu(const at::Tensor &t, const char *name) {
    TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

inline void hcheck(hipError_t e, const char *what) {
    TORCH_CHECK(e == hipSuccess, "hip ", what, ": ", hipGetErrorString(e));
}

// present and defined
inline bool has(const OptTensor &o) { return o && o->defined(); }

inline const uint16_t *bf16(const at::Tensor &t) { return reinterpret_cast<const uint16_t *>(t.data_ptr()); }
inline uint16_t *bf16_mut(const at::Tensor &t) { return reinterpret_cast<uint16_t *>(t.data_ptr()); }

// int64 -> int that refuses a value that does not fit (sizes, strides, paddings, variants)
inline int narrow(int64_t v, const char *op, const char *what) {
    TORCH_CHECK(v >= INT_MIN && v <= INT_MAX, op, ": ", what, " must be a 32-bit integer, got ", v);
    return static_cast<int>(v);
}

inline bool on_dev(const at::Tensor &t, const Dev &dev) { return dev ? t.device() == *dev : t.is_cuda(); }
inline const char *where(const Dev &dev) { return dev ? "on the leading tensor's device" : "on a GPU"; }

// 4-D channels_last tensor of `dt` on `dev`
inline void check_cl4(const at::Tensor &t, const char *op, const char *name, const Dev &dev,
                      at::ScalarType dt = at::kBFloat16) {
    TORCH_CHECK(t.dim() == 4 && t.scalar_type() == dt && t.is_contiguous(at::MemoryFormat::ChannelsLast) &&
                    on_dev(t, dev),
                op, ": ", name, " must be a 4-D channels_last ", dt, " tensor ", where(dev));
}

// ... of the shape {N, C, H, W}
inline void check_cl4(const at::Tensor &t, const char *op, const char *name, const Dev &dev, at::IntArrayRef nchw,
                      at::ScalarType dt = at::kBFloat16) {
    TORCH_CHECK(t.dim() == 4 && t.scalar_type() == dt && t.is_contiguous(at::MemoryFormat::ChannelsLast) &&
                    on_dev(t, dev) && t.sizes() == nchw,
                op, ": ", name, " must be a ", nchw, " channels_last ", dt, " tensor ", where(dev));
}

// the {N, C, H, W} of a checked 4-D tensor as ints
struct Dims4 {
    int n, c, h, w;
};
inline Dims4 dims4(const at::Tensor &t, const char *op, const char *name) {
    return {narrow(t.size(0), op, name), narrow(t.size(1), op, name), narrow(t.size(2), op, name),
            narrow(t.size(3), op, name)};
}

// contiguous 1-D / 2-D operand (bias, coefficient vector, mask, argmax bytes, packed weight) of `dt` with
// numel (at_least: or more) elements on `dev`
inline void check_dense(const at::Tensor &t, const char *op, const char *name, const Dev &dev, at::ScalarType dt,
                        int64_t numel, bool at_least = false) {
    TORCH_CHECK(t.scalar_type() == dt && t.is_contiguous() && (at_least ? t.numel() >= numel : t.numel() == numel) &&
                    on_dev(t, dev),
                op, ": ", name, " must be a contiguous ", dt, " tensor of ", at_least ? "at least " : "", numel,
                " elements ", where(dev));
}

// The f64 kStatSlots x 2 x C statistics workspace of the conv / GEMM / stem epilogues and the BNs that
// consume it; null when the argument is absent.
inline double *stats_ptr(const OptTensor &o, const char *op, int64_t C, const Dev &dev, const char *name = "stats") {
    if (!has(o)) return nullptr;
    check_dense(*o, op, name, dev, at::kDouble, kfk::kStatSlots * 2 * C);
    return o->data_ptr<double>();
}

// The kernels index with 32-bit offsets: the product of dims stays below 2^31.
inline void check_extent32(const char *op, const char *name, std::initializer_list<int64_t> dims) {
    int64_t n = 1;
    for (int64_t d : dims) {
        TORCH_CHECK(d >= 0 && d <= INT_MAX, op, ": ", name, " too large for 32-bit offsets");
        n *= d;
        TORCH_CHECK(n <= INT_MAX, op, ": ", name, " too large for 32-bit offsets");
    }
}

// The BN-backward epilogue of the conv kernels: the output (of y_sizes, K channels) is the gradient of a
// BN(+ReLU) output whose input is bn_x; `stats` receives sum(dz), sum(dz * x), the ReLU gate coming from
// bn_mask (one bit per element) or bn_fcoef (the forward [scale; shift]).  Fills ea and returns
// kEpiBwdBits or kEpiBwdCoef; 0 (ea untouched) without bn_x.
inline int bn_bwd_epilogue(const char *op, kfk::EpiArgs &ea, at::IntArrayRef y_sizes, int64_t K, const Dev &dev,
                           double *stats, const OptTensor &bn_x, const OptTensor &bn_fcoef, const OptTensor &bn_mask) {
    if (!has(bn_x)) return 0;
    TORCH_CHECK(stats, op, ": stats must be given with bn_x (it receives the BN-backward sums)");
    check_cl4(*bn_x, op, "bn_x", dev, y_sizes);
    ea.stats = stats;
    ea.bx = bf16(*bn_x);
    if (has(bn_mask)) {
        check_dense(*bn_mask, op, "bn_mask", dev, at::kByte, c10::multiply_integers(y_sizes) / 8);
        ea.bmask = bn_mask->data_ptr<uint8_t>();
        return kfk::kEpiBwdBits;
    }
    TORCH_CHECK(has(bn_fcoef), op, ": bn_fcoef must be given with bn_x (forward [scale; shift], f32) unless bn_mask is");
    check_dense(*bn_fcoef, op, "bn_fcoef", dev, at::kFloat, 2 * K, true);
    ea.fcoef = bn_fcoef->data_ptr<float>();
    return kfk::kEpiBwdCoef;
}

// The optional destination `out` (checked: `sizes`, the dtype / device / memory format of `opt`), else a new
// tensor; second: whether it was supplied.  Dense (not channels_last) destinations are checked by numel.
inline std::pair<at::Tensor, bool> out_or_empty(const OptTensor &out, at::IntArrayRef sizes, const at::TensorOptions &opt,
                                                const char *op, const char *name = "out") {
    if (!has(out)) return {at::empty(sizes, opt), false};
    const auto dt = c10::typeMetaToScalarType(opt.dtype());
    if (opt.memory_format_opt() == at::MemoryFormat::ChannelsLast) check_cl4(*out, op, name, opt.device(), sizes, dt);
    else check_dense(*out, op, name, opt.device(), dt, c10::multiply_integers(sizes));
    return {*out, true};
}

}  // namespace kfb
