// Pooling and bias + activation on NHWC bf16 tensors.
#include "bind_util.hpp"

#include <tuple>
#include <vector>

using namespace kfb;

namespace {

const auto kCL = at::MemoryFormat::ChannelsLast;

void check_bias_act(const at::Tensor &y, const char *op, const char *name) {
    check_cl4(y, op, name, kAnyGpu);
    TORCH_CHECK(kfk::bias_act_supported(y.size(1)), op, ": ", name, " must have C/8 a power of two <= 256");
}

// y = relu(y + bias) in place (relu=false: y += bias); bias f32 [C]
void bias_act_forward_(at::Tensor y, at::Tensor bias, bool relu) {
    const char *op = "bias_act_forward_";
    check_bias_act(y, op, "y");
    check_dense(bias, op, "bias", y.device(), at::kFloat, y.size(1));
    c10::DeviceGuard gd(y.device());
    const int C = narrow(y.size(1), op, "y");
    kfk::launch_bias_act_forward(bf16_mut(y), bias.data_ptr<float>(), y.numel() / C, C, relu, stream_of(y, 0));
}

// (dz, dbias): dz = dy * (y > 0) (relu; dz is dy itself without relu), dbias = sum dz over N, H, W (f32)
std::vector<at::Tensor> bias_act_backward(at::Tensor dy, at::Tensor y, bool relu) {
    const char *op = "bias_act_backward";
    check_bias_act(y, op, "y");
    check_cl4(dy, op, "dy", y.device(), y.sizes());
    c10::DeviceGuard gd(y.device());
    const int C = narrow(y.size(1), op, "y");
    const int64_t rows = y.numel() / C;
    at::Tensor dz = relu ? at::empty_like(dy, dy.options().memory_format(kCL)) : dy;
    at::Tensor db = at::empty({C}, y.options().dtype(at::kFloat));
    at::Tensor part = at::empty({std::max(1, kfk::bias_act_backward_blocks(rows, C)), C}, y.options().dtype(at::kFloat));
    kfk::launch_bias_act_backward(bf16(dy), bf16(y), bf16_mut(dz), db.data_ptr<float>(), part.data_ptr<float>(), rows, C,
                                  relu, stream_of(y, 0));
    return {dz, db};
}

// channels_last bf16 GPU tensor with C % 8 == 0: its {N, C, H, W}
Dims4 pool_in(const at::Tensor &x, const char *op, const char *name) {
    check_cl4(x, op, name, kAnyGpu);
    TORCH_CHECK(x.size(1) % 8 == 0, op, ": ", name, " must have C % 8 == 0");
    return dims4(x, op, name);
}

at::Tensor maxpool2x2_forward(at::Tensor x) {
    const char *op = "maxpool2x2_forward";
    const auto [N, C, H, W] = pool_in(x, op, "x");
    TORCH_CHECK(H % 2 == 0 && W % 2 == 0, "maxpool2x2_forward: x must have even H, W");
    c10::DeviceGuard gd(x.device());
    auto y = at::empty({N, C, H / 2, W / 2}, x.options().memory_format(kCL));
    kfk::launch_maxpool2x2_forward(bf16(x), bf16_mut(y), N, H, W, C, stream_of(x, 0));
    return y;
}

at::Tensor maxpool2x2_backward(at::Tensor x, at::Tensor dy, OptTensor gate_stats) {
    const char *op = "maxpool2x2_backward";
    const auto [N, C, H, W] = pool_in(x, op, "x");
    TORCH_CHECK(H % 2 == 0 && W % 2 == 0, "maxpool2x2_backward: x must have even H, W");
    double *gs = stats_ptr(gate_stats, op, C, x.device(), "gate_stats");
    check_cl4(dy, op, "dy", x.device(), {N, C, H / 2, W / 2});
    c10::DeviceGuard gd(x.device());
    auto dx = at::empty_like(x, x.options().memory_format(kCL));
    kfk::launch_maxpool2x2_backward(bf16(x), bf16(dy), bf16_mut(dx), N, H, W, C, stream_of(x, 0), gs);
    return dx;
}

std::tuple<at::Tensor, at::Tensor> maxpool3s2_forward(at::Tensor x, int64_t pad) {
    const char *op = "maxpool3s2_forward";
    const auto [N, C, H, W] = pool_in(x, op, "x");
    TORCH_CHECK(H >= 3 && W >= 3, "maxpool3s2_forward: x must have H, W >= 3");
    TORCH_CHECK(pad == 0 || pad == 1, "maxpool3s2_forward: pad must be 0 or 1");
    c10::DeviceGuard gd(x.device());
    const int p = static_cast<int>(pad), OH = kfk::maxpool3s2_out(H, p), OW = kfk::maxpool3s2_out(W, p);
    auto y = at::empty({N, C, OH, OW}, x.options().memory_format(kCL));
    auto arg = at::empty({N, OH, OW, C}, x.options().dtype(at::kByte));
    kfk::launch_maxpool3s2_forward(bf16(x), bf16_mut(y), arg.data_ptr<uint8_t>(), N, H, W, C, p, stream_of(x, 0));
    return {y, arg};
}

at::Tensor maxpool3s2_backward(at::Tensor dy, at::Tensor arg, int64_t H, int64_t W, int64_t pad) {
    const char *op = "maxpool3s2_backward";
    const auto [N, C, OH, OW] = pool_in(dy, op, "dy");
    const int h = narrow(H, op, "H"), w = narrow(W, op, "W"), p = narrow(pad, op, "pad");
    TORCH_CHECK(OH == kfk::maxpool3s2_out(h, p) && OW == kfk::maxpool3s2_out(w, p),
                "maxpool3s2_backward: dy must be the pooled gradient of an H x W input");
    check_dense(arg, op, "arg", dy.device(), at::kByte, dy.numel());
    c10::DeviceGuard gd(dy.device());
    auto dx = at::empty({N, C, h, w}, dy.options().memory_format(kCL));
    kfk::launch_maxpool3s2_backward(bf16(dy), arg.data_ptr<uint8_t>(), bf16_mut(dx), N, h, w, C, p, stream_of(dy, 0));
    return dx;
}

// Global average pool of a channels_last bf16 [N, C, H, W] -> [N, C] bf16 (and its backward).
at::Tensor global_avgpool_forward(at::Tensor x) {
    const char *op = "global_avgpool_forward";
    const auto [N, C, H, W] = pool_in(x, op, "x");
    c10::DeviceGuard gd(x.device());
    auto y = at::empty({N, C}, x.options());
    kfk::launch_global_avgpool_forward(bf16(x), bf16_mut(y), N, narrow(int64_t(H) * W, op, "H * W"), C, stream_of(x, 0));
    return y;
}

at::Tensor global_avgpool_backward(at::Tensor dy, int64_t H, int64_t W) {
    const char *op = "global_avgpool_backward";
    TORCH_CHECK(dy.is_cuda() && dy.scalar_type() == at::kBFloat16 && dy.dim() == 2 && dy.size(1) % 8 == 0 &&
                    H > 0 && W > 0,
                "global_avgpool_backward: dy must be a bf16 [N, C] GPU tensor with C % 8 == 0");
    const int hw = narrow(H * W, op, "H * W"), C = narrow(dy.size(1), op, "dy");
    dy = dy.contiguous();
    c10::DeviceGuard gd(dy.device());
    auto dx = at::empty({dy.size(0), C, H, W}, dy.options().memory_format(kCL));
    kfk::launch_global_avgpool_backward(bf16(dy), bf16_mut(dx), dy.size(0), hw, C, stream_of(dy, 0));
    return dx;
}

at::Tensor avgpool3s1(at::Tensor x) {
    const char *op = "avgpool3s1";
    const auto [N, C, H, W] = pool_in(x, op, "x");
    TORCH_CHECK(H >= 3 && W >= 3, "avgpool3s1: x must have H, W >= 3");
    c10::DeviceGuard gd(x.device());
    auto y = at::empty_like(x, x.options().memory_format(kCL));
    kfk::launch_avgpool3s1(bf16(x), bf16_mut(y), N, H, W, C, stream_of(x, 0));
    return y;
}

}  // namespace

void bind_pool_act(py::module_ &m) {
    m.def("bias_act_supported", &kfk::bias_act_supported);
    m.def("bias_act_forward_", &bias_act_forward_, "y = relu(y + bias) in place (NHWC bf16, f32 bias)",
          py::arg("y"), py::arg("bias"), py::arg("relu") = true);
    m.def("bias_act_backward", &bias_act_backward, "(dy * (y > 0), its per-channel sum) in one pass",
          py::arg("dy"), py::arg("y"), py::arg("relu") = true);
    m.def("maxpool2x2_forward", &maxpool2x2_forward, "2x2/s2 max-pool, NHWC bf16 (no argmax tensor)");
    m.def("maxpool2x2_backward", &maxpool2x2_backward, "2x2/s2 max-pool gradient (gather from x, dy); gate_stats: "
          "x is a ReLU output, also gate by x > 0 and sum the result per channel", py::arg("x"), py::arg("dy"),
          py::arg("gate_stats") = py::none());
    m.def("maxpool3s2_forward", &maxpool3s2_forward, "3x3/s2 max-pool (pad 0/1), NHWC bf16 -> (y, argmax bytes)");
    m.def("maxpool3s2_backward", &maxpool3s2_backward, "3x3/s2 max-pool gradient (gather via the argmax bytes)");
    m.def("global_avgpool_forward", &global_avgpool_forward, "global average pool, NHWC bf16 -> [N, C]");
    m.def("global_avgpool_backward", &global_avgpool_backward, "global average pool backward -> NHWC bf16",
          py::arg("dy"), py::arg("H"), py::arg("W"));
    m.def("avgpool3s1", &avgpool3s1, "3x3/s1/p1 average pool, count_include_pad (also its own gradient on dy)");
}
