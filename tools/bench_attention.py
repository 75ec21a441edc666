"""Fused attention (attention.hip, attention_long.hip) at BERT-base shapes: forward and backward
kernel time per call (median of 20, events), 12 heads x 64, dropout p = 0.1 and 0, plus the HBM
bytes each must move (qkv in, out + lse out; backward: qkv, out, dout in, dqkv out) and the
resulting fraction of a 5.3 TB/s streaming roofline.  Next to it the time of what the fused path
replaces: ``ops.attention.self_attention`` on its SDPA fallback (``KUNGFU_ATTN_LONG=0`` for
S > 128), head permutes, transposed output copy and dq/dk/dv concatenation included.

    python tools/bench_attention.py [calls] [--batch 128] [--seq 128] [--heads 12]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kungfu_amd._lib import hip  # noqa: E402
from kungfu_amd.ops import attention as attn  # noqa: E402


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


def sdpa_fallback(qkv, dout, NH, p, n):
    """(forward us, backward us) of self_attention with the fused kernels switched off."""
    fused = attn.eligible
    attn.eligible = lambda *a: False  # as KUNGFU_ATTN_LONG=0 does for S > 128, here for any S
    try:
        q = qkv.clone().requires_grad_(True)
        y = attn.self_attention(q, NH, p)
        assert type(y.grad_fn).__name__ != "_AttnFnBackward"
        tf = med(lambda: attn.self_attention(q, NH, p), n)
        tb = med(lambda: torch.autograd.grad(y, q, dout, retain_graph=True), n)
    finally:
        attn.eligible = fused
    return tf, tb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("calls", nargs="?", type=int, default=20, help="calls to time")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--heads", type=int, default=12)
    args = ap.parse_args()
    n = args.calls
    H = hip()
    B, S, NH = args.batch, args.seq, args.heads
    D = NH * 64
    torch.manual_seed(0)
    qkv = (torch.randn(B, S, 3 * D, device="cuda") * 0.5).bfloat16()
    dout = (torch.randn(B, S, D, device="cuda") * 0.1).bfloat16()
    scale = 64 ** -0.5
    print("B=%d S=%d H=%d" % (B, S, NH), flush=True)
    for p in (0.1, 0.0):
        out, lse = H.attention_forward(qkv, NH, scale, 1234, p)
        tf = med(lambda: H.attention_forward(qkv, NH, scale, 1234, p), n)
        tb = med(lambda: H.attention_backward(qkv, out, lse, dout, NH, scale, 1234, p), n)
        fb = qkv.numel() * 2 + out.numel() * 2 + lse.numel() * 4
        bb = qkv.numel() * 2 * 2 + out.numel() * 2 * 2 + lse.numel() * 4
        sf, sb = sdpa_fallback(qkv, dout, NH, p, n)
        print("p=%.1f  fwd %6.1f us (%.0f %% of roofline %.1f us)  bwd %6.1f us (%.0f %% of roofline %.1f us)"
              "  |  SDPA fallback fwd %6.1f us  bwd %6.1f us  |  fwd+bwd fused / fallback %.2f" % (
                  p, tf, 100 * fb / 5.3e6 / tf, fb / 5.3e6, tb, 100 * bb / 5.3e6 / tb, bb / 5.3e6, sf, sb,
                  (tf + tb) / (sf + sb)), flush=True)


if __name__ == "__main__":
    main()
