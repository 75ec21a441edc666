"""Fused residual-add + RMSNorm (rmsnorm.hip) and SwiGLU (swiglu.hip) against the torch compositions they replace, at
LLaMA shapes: 8192 tokens, row lengths D in {1024, 4096, 8192}, FFN widths F in {2816, 11008}.

Per operation and direction the variants alternate over ``--rounds`` rounds in this one process, each timed as the
median of ``calls`` event-timed calls: ``fused`` and ``fused again`` (the same call twice per round: their ratio is the
run-to-run spread) and ``torch`` (``ops.rmsnorm._ENABLED = False`` / ``ops.swiglu._ENABLED = False``: the composition in
f32 on the bf16 tensors, as bf16 autocast runs it).  The forward is the op called on tensors that require grad, the
backward ``torch.autograd.grad`` through it, both routes alike.  Next to the fused medians: the HBM bytes the operation
must move (RMSNorm forward x, r in and s, y out; backward dy, ds_in, s in and ds out; SwiGLU forward gu in and h out;
backward dh, gu in and dgu out; gamma, rstd and the dgamma partials left out) and the share of a 5.3 TB/s streaming rate
they amount to.

    python tools/bench_llama_block.py [calls] [--tokens 8192] [--rounds 5] [--dims 1024,4096,8192] [--ffn 2816,11008]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kungfu_amd.ops import rmsnorm as rn, swiglu as sw  # noqa: E402

HBM = 5.3e6  # bytes per microsecond


def med(fn, n):
    ts = []
    for _ in range(3):
        fn()
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def routed(mod, enabled, fn):
    """``fn`` with the module's switch set, restored afterwards."""
    def call(*a):
        mod._ENABLED = enabled
        try:
            return fn(*a)
        finally:
            mod._ENABLED = True
    return call


def compare(tag, mod, fused_name, op, inputs, gouts, fwd_bytes, bwd_bytes, args):
    """Alternate the variants of one operation and print the medians, the spread and the fused route's HBM share."""
    variants = {}
    for name, enabled in (("fused", True), ("torch", False)):
        f = routed(mod, enabled, op)
        leaves = [t.clone().requires_grad_(True) for t in inputs]
        outs = f(*leaves)
        outs = outs if isinstance(outs, tuple) else (outs,)
        assert (type(outs[0].grad_fn).__name__ == fused_name) == enabled, (name, outs[0].grad_fn)
        variants[name] = (lambda f=f, leaves=leaves: f(*leaves),
                          lambda outs=outs, leaves=leaves: torch.autograd.grad(outs, leaves, gouts, retain_graph=True))
    variants = {"fused": variants["fused"], "fused again": variants["fused"], "torch": variants["torch"]}
    ts = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, (f, b) in variants.items():
            ts[k].append((med(f, args.calls), med(b, args.calls)))
    m = {}
    for k, v in ts.items():
        fs, bs = sorted(f for f, _ in v), sorted(b for _, b in v)
        m[k] = (fs[len(fs) // 2], bs[len(bs) // 2])
        print("%s  %-11s fwd %7.1f us (min %7.1f max %7.1f)  bwd %7.1f us (min %7.1f max %7.1f) over %d rounds" % (
            tag, k, m[k][0], fs[0], fs[-1], m[k][1], bs[0], bs[-1], len(v)), flush=True)
    for i, (d, nbytes) in enumerate((("fwd", fwd_bytes), ("bwd", bwd_bytes))):
        t = m["fused"][i]
        print("%s  %s: fused / torch %.3f   fused again / fused %.3f   %.2f TB/s of %d bytes, %.0f %% of 5.3 TB/s" % (
            tag, d, t / m["torch"][i], m["fused again"][i] / t, nbytes / t / 1e6, nbytes, 100 * nbytes / HBM / t),
            flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("calls", nargs="?", type=int, default=20, help="calls per timing")
    ap.add_argument("--tokens", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=5, help="rounds the variants alternate over")
    ap.add_argument("--dims", default="1024,4096,8192", help="RMSNorm row lengths")
    ap.add_argument("--ffn", default="2816,11008", help="SwiGLU widths F")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_llama_block: needs a GPU")
    T = args.tokens
    torch.manual_seed(0)
    for D in (int(d) for d in args.dims.split(",")):
        x, r, dy, ds = ((torch.randn(T, D, device="cuda") * 0.5).bfloat16() for _ in range(4))
        w = torch.rand(D, device="cuda") + 0.5
        compare("rmsnorm T=%d D=%d" % (T, D), rn, "_AddRMSNormFnBackward", lambda a, b, c: rn.add_rms_norm(a, b, c, 1e-6),
                (x, r, w), (dy, ds), 4 * T * D * 2, 4 * T * D * 2, args)
    for F in (int(f) for f in args.ffn.split(",")):
        gu = (torch.randn(T, 2 * F, device="cuda") * 1.5).bfloat16()
        dh = (torch.randn(T, F, device="cuda") * 0.5).bfloat16()
        compare("swiglu  T=%d F=%d" % (T, F), sw, "_SwiGLUFnBackward", sw.swiglu, (gu,), (dh,), 3 * T * F * 2,
                5 * T * F * 2, args)


if __name__ == "__main__":
    main()
