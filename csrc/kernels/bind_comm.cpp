// Communication: HIP IPC buffers, the collective-interference emulator, device links, the RCCL controller and
// its watchdog, the pair-averaging prefetcher and the native backtrace handler.
#include "bind_util.hpp"
#include "rccl_comm.hpp"

#include <csignal>
#include <cstring>
#include <execinfo.h>
#include <memory>
#include <tuple>
#include <unistd.h>
#include <vector>

using namespace kfb;

namespace {

// ---- device model store: HIP IPC export / import ------------------------------------
// A dedicated hipMalloc allocation (not a caching-allocator sub-block) so the
// IPC handle maps exactly this buffer; peers open it and pull over xGMI with
// no participation of the owner (one-sided, like the reference's P2P store).

at::Tensor ipc_alloc(int64_t numel, int64_t device) {
    c10::DeviceGuard gd(at::Device(at::kCUDA, device));
    void *p = nullptr;
    hcheck(hipMalloc(&p, std::max<int64_t>(numel, 1) * 4), "Malloc");
    hcheck(hipMemset(p, 0, std::max<int64_t>(numel, 1) * 4), "Memset");
    auto opts = at::TensorOptions().dtype(at::kFloat).device(at::kCUDA, device);
    return torch::from_blob(p, {numel}, [](void *q) { (void)hipFree(q); }, opts);
}

py::bytes ipc_handle(at::Tensor t) {
    hipIpcMemHandle_t h;
    hcheck(hipIpcGetMemHandle(&h, t.data_ptr()), "IpcGetMemHandle");
    return py::bytes(reinterpret_cast<const char *>(&h), sizeof(h));
}

at::Tensor ipc_open(py::bytes handle, int64_t numel, int64_t device) {
    std::string hs = handle;
    TORCH_CHECK(hs.size() == sizeof(hipIpcMemHandle_t), "ipc_open: bad handle size");
    hipIpcMemHandle_t h;
    std::memcpy(&h, hs.data(), sizeof(h));
    c10::DeviceGuard gd(at::Device(at::kCUDA, device));
    void *p = nullptr;
    hcheck(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess), "IpcOpenMemHandle");
    auto opts = at::TensorOptions().dtype(at::kFloat).device(at::kCUDA, device);
    return torch::from_blob(p, {numel}, [](void *q) { (void)hipIpcCloseMemHandle(q); }, opts);
}

// Collective-interference emulator (comm_emu.hip): stands in for one all-reduce of `bucket`.
void comm_emulate(at::Tensor bucket, at::Tensor scratch, int64_t traffic_bytes, int64_t ctas, double seconds,
                  int64_t stream) {
    check_gpu(bucket, "bucket");
    check_gpu(scratch, "scratch");
    const int64_t bytes = bucket.numel() * bucket.element_size();
    TORCH_CHECK(scratch.numel() * scratch.element_size() >= bytes, "comm_emulate: scratch smaller than the bucket");
    TORCH_CHECK(bytes >= 16 && reinterpret_cast<uintptr_t>(bucket.data_ptr()) % 16 == 0 &&
                    reinterpret_cast<uintptr_t>(scratch.data_ptr()) % 16 == 0,
                "comm_emulate: 16-byte aligned buffers of >= 16 bytes");
    c10::DeviceGuard gd(bucket.device());
    kfk::launch_comm_emulate(bucket.data_ptr(), scratch.data_ptr(), bytes, traffic_bytes, static_cast<int>(ctas),
                             seconds, stream_of(bucket, stream));
}

// Peer access / link of `device` to every visible device (the bench pre-flight's P2P
// matrix): (peer, can_access_peer, link type, hop count); link type per
// hipExtGetLinkTypeAndHopCount (HSA_AMD_LINK_INFO_TYPE_*: 4 = xGMI, 2 = PCIe).
std::vector<std::tuple<int, int, int, int>> device_links(int64_t device) {
    int n = 0;
    hcheck(hipGetDeviceCount(&n), "GetDeviceCount");
    std::vector<std::tuple<int, int, int, int>> out;
    for (int p = 0; p < n; ++p) {
        if (p == device) continue;
        int can = 0;
        uint32_t lt = 0, hops = 0;
        if (hipDeviceCanAccessPeer(&can, static_cast<int>(device), p) != hipSuccess) can = -1;
        if (hipExtGetLinkTypeAndHopCount(static_cast<int>(device), p, &lt, &hops) != hipSuccess) lt = hops = 0;
        out.emplace_back(p, can, static_cast<int>(lt), static_cast<int>(hops));
    }
    return out;
}

// ---- RCCL --------------------------------------------------------------------------

class Comm {
  public:
    Comm(py::bytes id, int rank, int size, int device, double init_timeout_s, int min_ctas, int max_ctas) {
        std::string sid(id);
        py::gil_scoped_release nogil;  // init polls its deadline; other threads keep running
        c_.reset(new kfk::RcclComm(sid, rank, size, device, init_timeout_s, min_ctas, max_ctas));
    }
    py::tuple ctas() const { return py::make_tuple(c_->min_ctas(), c_->max_ctas()); }
    int rank() const { return c_->rank(); }
    int size() const { return c_->size(); }
    bool valid() const { return c_->valid(); }
    bool blocking() const { return c_->blocking(); }
    void all_reduce(at::Tensor in, at::Tensor out, int64_t op, int64_t stream, const std::string &tag) {
        check_gpu(in, "in");
        check_gpu(out, "out");
        TORCH_CHECK(in.numel() == out.numel(), "all_reduce: size mismatch");
        py::gil_scoped_release nogil;  // enq may poll wait_ready (non-blocking comms)
        c_->all_reduce(in.data_ptr(), out.data_ptr(), in.numel(), dtype_code(in), static_cast<int>(op),
                       stream_of(in, stream), tag.c_str());
    }
    void broadcast(at::Tensor t, int64_t root, int64_t stream, const std::string &tag) {
        check_gpu(t, "t");
        py::gil_scoped_release nogil;  // enq may poll wait_ready (non-blocking comms)
        c_->broadcast(t.data_ptr(), t.data_ptr(), t.numel(), dtype_code(t), static_cast<int>(root),
                      stream_of(t, stream), tag.c_str());
    }
    void reduce(at::Tensor in, at::Tensor out, int64_t op, int64_t root, int64_t stream, const std::string &tag) {
        check_gpu(in, "in");
        py::gil_scoped_release nogil;  // enq may poll wait_ready (non-blocking comms)
        c_->reduce(in.data_ptr(), out.data_ptr(), in.numel(), dtype_code(in), static_cast<int>(op),
                   static_cast<int>(root), stream_of(in, stream), tag.c_str());
    }
    void all_gather(at::Tensor in, at::Tensor out, int64_t stream, const std::string &tag) {
        check_gpu(in, "in");
        check_gpu(out, "out");
        TORCH_CHECK(out.numel() == in.numel() * c_->size(), "all_gather: out must hold size*numel(in)");
        py::gil_scoped_release nogil;  // enq may poll wait_ready (non-blocking comms)
        c_->all_gather(in.data_ptr(), out.data_ptr(), in.numel(), dtype_code(in), stream_of(in, stream),
                       tag.c_str());
    }
    void reduce_scatter(at::Tensor in, at::Tensor out, int64_t op, int64_t stream, const std::string &tag) {
        check_gpu(in, "in");
        check_gpu(out, "out");
        TORCH_CHECK(in.numel() == out.numel() * c_->size(), "reduce_scatter: in must hold size*numel(out)");
        py::gil_scoped_release nogil;  // enq may poll wait_ready (non-blocking comms)
        c_->reduce_scatter(in.data_ptr(), out.data_ptr(), out.numel(), dtype_code(in), static_cast<int>(op),
                           stream_of(in, stream), tag.c_str());
    }
    void send(at::Tensor t, int64_t peer, int64_t stream) {
        check_gpu(t, "t");
        py::gil_scoped_release nogil;  // enq may poll wait_ready (non-blocking comms)
        c_->send(t.data_ptr(), t.numel(), dtype_code(t), static_cast<int>(peer), stream_of(t, stream));
    }
    void recv(at::Tensor t, int64_t peer, int64_t stream) {
        check_gpu(t, "t");
        py::gil_scoped_release nogil;  // enq may poll wait_ready (non-blocking comms)
        c_->recv(t.data_ptr(), t.numel(), dtype_code(t), static_cast<int>(peer), stream_of(t, stream));
    }
    void group_start() { c_->group_start(); }
    void group_end() {
        py::gil_scoped_release nogil;
        c_->group_end();
    }
    void watch(int64_t stream, const std::string &what) {
        c_->watch(reinterpret_cast<hipStream_t>(stream), what);
    }
    int async_error() { return c_->async_error(); }
    // Graph all-reduce on the device: one round = one grouped batch of send/recv
    // (kungfu::plan_graph_all_reduce), then the K1 reduce kernel for every received
    // partial (buf[off:off+len] = op(buf[...], scratch[sc:sc+len])).  Every rank must run
    // its own plan of the same strategy graphs (same rounds, matched ops).
    using Xfer = std::tuple<int, int, int64_t, int64_t, int64_t>;  // recv, peer, off, len, scratch
    void graph_run(at::Tensor buf, c10::optional<at::Tensor> scratch, const std::vector<std::vector<Xfer>> &rounds,
                   int64_t op, int64_t stream) {
        check_gpu(buf, "buf");
        TORCH_CHECK(buf.is_contiguous(), "graph_run: buf must be contiguous");
        const int dt = dtype_code(buf);
        const size_t esz = buf.element_size();
        auto *base = static_cast<uint8_t *>(buf.data_ptr());
        uint8_t *sbase = nullptr;
        int64_t sn = 0;
        if (has(scratch)) {
            TORCH_CHECK(scratch->is_cuda() && scratch->scalar_type() == buf.scalar_type() && scratch->is_contiguous() &&
                            scratch->device() == buf.device(),
                        "graph_run: scratch must be a contiguous tensor of buf's dtype on its device");
            sbase = static_cast<uint8_t *>(scratch->data_ptr());
            sn = scratch->numel();
        }
        const int64_t n = buf.numel();
        // validate the whole plan before issuing anything
        for (const auto &r : rounds)
            for (const auto &x : r) {
                const int64_t off = std::get<2>(x), len = std::get<3>(x), sc = std::get<4>(x);
                const int peer = std::get<1>(x);
                TORCH_CHECK(off >= 0 && len >= 0 && off + len <= n, "graph_run: range out of bounds");
                TORCH_CHECK(peer >= 0 && peer < c_->size() && peer != c_->rank(), "graph_run: bad peer");
                TORCH_CHECK(!std::get<0>(x) || sc < 0 || (sbase && sc + len <= sn), "graph_run: scratch too small");
            }
        c10::DeviceGuard gd(buf.device());
        auto s = stream_of(buf, stream);
        py::gil_scoped_release nogil;
        for (const auto &r : rounds) {
            if (r.empty()) continue;
            c_->group_start();
            for (const auto &x : r) {
                const int peer = std::get<1>(x);
                const int64_t off = std::get<2>(x), len = std::get<3>(x), sc = std::get<4>(x);
                if (std::get<0>(x)) {
                    uint8_t *dst = sc >= 0 ? sbase + sc * esz : base + off * esz;
                    c_->recv(dst, len, dt, peer, s);
                } else {
                    c_->send(base + off * esz, len, dt, peer, s);
                }
            }
            c_->group_end();
            for (const auto &x : r) {
                const int64_t off = std::get<2>(x), len = std::get<3>(x), sc = std::get<4>(x);
                if (std::get<0>(x) && sc >= 0)
                    kfk::launch_reduce(base + off * esz, base + off * esz, sbase + sc * esz, len, dt,
                                       static_cast<int>(op), s);
            }
        }
        c_->watch(s, "GraphAllReduce(" + std::to_string(rounds.size()) + " rounds, " + std::to_string(n) + " elems)");
    }
    void destroy() {
        py::gil_scoped_release nogil;
        c_->destroy();
    }
    void abort() { c_->abort(); }

  private:
    std::unique_ptr<kfk::RcclComm> c_;
};

// Native backtrace on SIGSEGV / SIGBUS / SIGABRT (KUNGFU_NATIVE_BACKTRACE=1, a debugging aid: Python's
// faulthandler shows only the Python frames of a crash inside RCCL / HIP).  Chains to the previous
// handler so faulthandler still prints its part.
struct sigaction g_prev_segv, g_prev_bus, g_prev_abrt;
void native_bt_handler(int sig, siginfo_t *info, void *uc) {
    static const char hdr[] = "\n[F] kungfu: native backtrace (signal):\n";
    (void)!write(2, hdr, sizeof(hdr) - 1);
    void *frames[64];
    const int n = backtrace(frames, 64);
    backtrace_symbols_fd(frames, n, 2);
    struct sigaction *prev = sig == SIGSEGV ? &g_prev_segv : sig == SIGBUS ? &g_prev_bus : &g_prev_abrt;
    sigaction(sig, prev, nullptr);
    if (prev->sa_flags & SA_SIGINFO) {
        if (prev->sa_sigaction) prev->sa_sigaction(sig, info, uc);
    } else if (prev->sa_handler != SIG_DFL && prev->sa_handler != SIG_IGN && prev->sa_handler) {
        prev->sa_handler(sig);
    }
    raise(sig);
}
void install_native_backtrace() {
    struct sigaction sa;
    std::memset(&sa, 0, sizeof(sa));
    sa.sa_sigaction = native_bt_handler;
    sa.sa_flags = SA_SIGINFO | SA_ONSTACK;
    sigemptyset(&sa.sa_mask);
    sigaction(SIGSEGV, &sa, &g_prev_segv);
    sigaction(SIGBUS, &sa, &g_prev_bus);
    sigaction(SIGABRT, &sa, &g_prev_abrt);
}
}  // namespace

void bind_comm(py::module_ &m) {
    m.def("install_native_backtrace", &install_native_backtrace,
          "print a native backtrace to stderr on SIGSEGV/SIGBUS/SIGABRT (chains to the previous handler)");
    m.def("ipc_alloc", &ipc_alloc, "dedicated f32 device buffer exportable over HIP IPC");
    m.def("ipc_handle", &ipc_handle, "HIP IPC handle (64 bytes) of an ipc_alloc buffer");
    m.def("ipc_open", &ipc_open, "map a peer's exported buffer as an f32 tensor");
    m.def("comm_emulate", &comm_emulate, py::arg("bucket"), py::arg("scratch"), py::arg("traffic_bytes"),
          py::arg("ctas"), py::arg("seconds"), py::arg("stream") = 0,
          "local footprint of one all-reduce: ctas workgroups stream traffic_bytes, resident for seconds");
    m.def("device_links", &device_links, py::arg("device"),
          "[(peer, can_access_peer, link_type, hops)] of `device` to every other visible device");
    m.def("rccl_unique_id", [] { return py::bytes(kfk::RcclComm::unique_id()); });
    m.def("rccl_version", &kfk::RcclComm::version);
    m.def("rccl_watchdog_info", [] {
        const auto i = kfk::watchdog_info();
        py::dict d;
        d["registered"] = i.registered;
        d["completed"] = i.completed;
        d["pending"] = i.pending;
        d["oldest_s"] = i.oldest_s;
        d["timeout_s"] = i.timeout_s;
        d["abort_on_stall"] = i.abort_on_stall;
        d["stalls_logged"] = i.stalls_logged;
        return d;
    });
    kfk::watchdog_set_freeze_hook([] {
        if (Py_IsInitialized()) PyGILState_Ensure();  // held until the process exits
    });
    m.def("rccl_watchdog_set_label", &kfk::watchdog_set_label);
    m.def("rccl_watchdog_set_timeout", &kfk::watchdog_set_timeout);
    py::class_<kfk::PairPrefetcher>(m, "PairPrefetcher",
                                    "native prefetch thread of the pair-averaging peer model (pair_prefetch.hip)")
        .def(py::init<const std::string &, int, int, const std::string &, const std::string &, int64_t, int>(),
             py::arg("libpath"), py::arg("device"), py::arg("self_rank"), py::arg("rec_name"), py::arg("model_name"),
             py::arg("nbytes"), py::arg("slots") = 3)
        .def(
            "start",
            [](kfk::PairPrefetcher &p, uintptr_t pending_ev, int64_t pending_ver, uintptr_t host_copy, int target,
               std::vector<uintptr_t> src_slots, int64_t own_ver, uintptr_t dst, uintptr_t after_ev,
               uintptr_t host_stage) {
                kfk::PairPrefetcher::Job j;
                j.pending_ev = pending_ev, j.pending_ver = pending_ver, j.host_copy = host_copy, j.target = target;
                j.src_slots = std::move(src_slots), j.own_ver = own_ver, j.dst = dst, j.after_ev = after_ev;
                j.host_stage = host_stage;
                py::gil_scoped_release nogil;  // waits for the previous job
                p.start(j);
            },
            py::arg("pending_ev"), py::arg("pending_ver"), py::arg("host_copy"), py::arg("target"),
            py::arg("src_slots"), py::arg("own_ver"), py::arg("dst"), py::arg("after_ev"), py::arg("host_stage"))
        .def("busy", &kfk::PairPrefetcher::busy)
        .def(
            "finish",
            [](kfk::PairPrefetcher &p, uintptr_t wait_stream) {
                kfk::PairPrefetcher::Result r;
                {
                    py::gil_scoped_release nogil;
                    r = p.finish(wait_stream);
                }
                if (!r.error.empty()) throw std::runtime_error(r.error);
                return py::make_tuple(r.status, r.version, r.own_ver);
            },
            py::arg("wait_stream"), "join the job: (status 0 none / 1 pulled / 2 dropped, version, own advertised version)");

    py::class_<Comm>(m, "RcclComm")
        .def(py::init<py::bytes, int, int, int, double, int, int>(), py::arg("uid"), py::arg("rank"),
             py::arg("size"), py::arg("device"), py::arg("init_timeout_s") = 0.0, py::arg("min_ctas") = 0,
             py::arg("max_ctas") = 0)
        .def("ctas", &Comm::ctas, "(min, max) CTA budget of this communicator (0 = RCCL default)")
        .def("rank", &Comm::rank)
        .def("size", &Comm::size)
        .def("valid", &Comm::valid)
        .def("blocking", &Comm::blocking)
        .def("all_reduce", &Comm::all_reduce, py::arg("input"), py::arg("output"), py::arg("op") = 0,
             py::arg("stream") = 0, py::arg("tag") = "")
        .def("broadcast", &Comm::broadcast, py::arg("tensor"), py::arg("root") = 0, py::arg("stream") = 0,
             py::arg("tag") = "")
        .def("reduce", &Comm::reduce, py::arg("input"), py::arg("output"), py::arg("op") = 0, py::arg("root") = 0,
             py::arg("stream") = 0, py::arg("tag") = "")
        .def("all_gather", &Comm::all_gather, py::arg("input"), py::arg("output"), py::arg("stream") = 0,
             py::arg("tag") = "")
        .def("reduce_scatter", &Comm::reduce_scatter, py::arg("input"), py::arg("output"), py::arg("op") = 0,
             py::arg("stream") = 0, py::arg("tag") = "")
        .def("group_start", &Comm::group_start)
        .def("group_end", &Comm::group_end)
        .def("watch", &Comm::watch, py::arg("stream"), py::arg("what"))
        .def("async_error", &Comm::async_error)
        .def("send", &Comm::send, py::arg("tensor"), py::arg("peer"), py::arg("stream") = 0)
        .def("recv", &Comm::recv, py::arg("tensor"), py::arg("peer"), py::arg("stream") = 0)
        .def("graph_run", &Comm::graph_run, "grouped send/recv rounds + K1 reduce (device graph all-reduce)",
             py::arg("buf"), py::arg("scratch"), py::arg("rounds"), py::arg("op") = 0, py::arg("stream") = 0)
        .def("destroy", &Comm::destroy)
        .def("abort", &Comm::abort);
}
