// torch binding of the CDNA4 kernels and the RCCL controller: kungfu_amd._hip
//
// Every op enqueues on the current HIP stream of the tensor's device (or an
// explicit stream handle) and never synchronises the host.  One bind_<family>.cpp per kernel
// family holds the wrappers and their m.def lines; bind_util.hpp holds the argument checks they share.
#include <torch/extension.h>

void bind_flat(py::module_ &m);
void bind_conv(py::module_ &m);
void bind_bn(py::module_ &m);
void bind_stem(py::module_ &m);
void bind_pool_act(py::module_ &m);
void bind_bert(py::module_ &m);
void bind_comm(py::module_ &m);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.doc() = "kungfu-amd CDNA4 kernels (gfx950) and RCCL controller";
    bind_flat(m);
    bind_conv(m);
    bind_bn(m);
    bind_stem(m);
    bind_pool_act(m);
    bind_bert(m);
    bind_comm(m);
}
