"""Fused attention (attention.hip, attention_long.hip) at BERT-base shapes: forward and backward
kernel time per call (median of 20, events), 12 heads x 64, dropout p = 0.1 and 0, plus the HBM
bytes each must move (qkv in, out + lse out; backward: qkv, out, dout in, dqkv out) and the
resulting fraction of a 5.3 TB/s streaming roofline.  Next to it the time of what the fused path
replaces: ``ops.attention.self_attention`` on its SDPA fallback (``KUNGFU_ATTN_LONG=0`` for
S > 128), head permutes, transposed output copy and dq/dk/dv concatenation included.

With ``--lengths`` (a fraction of S in (0, 1]: every sequence that long; or ``random``: seeded uniform
lengths in [1, S]) it times a padded batch instead, forward + backward per variant, the variants
alternating over ``--rounds`` rounds in this one process: the fused call without lengths twice (``full``
and ``full again``: their difference is the run-to-run spread), the length-aware kernels
(attention_lengths.hip) and the SDPA path a masked batch took before them (BertLayer's: head permutes, a
boolean key mask, transposed output copy, dq/dk/dv concatenation).

With ``--causal`` it times the causal kernels (attention_causal.hip), forward and backward separately, the variants
alternating the same way: the causal call in its heaviest-first workgroup order and in the plain order, the
bidirectional call at the same shape twice (S <= 512) and the SDPA ``is_causal=True`` path with BertLayer's permutes
and copies.

With ``--head-dim 128`` it times the head dim 128 kernels (attention_d128.hip) on multi-head attention, forward and
backward separately, bidirectional or (``--causal``) causal, twice per round, against the SDPA path at the same head dim
with the permutes, copy and concatenation.

With ``--head-dim 128 --kv-heads N`` it times the same kernels on grouped-query heads against the two ways to serve
the call without grouping: K/V expanded to every query head plus the group sum of dk / dv, and the SDPA fallback.

With ``--head-dim 128 --rope BASE`` (with or without ``--kv-heads``) it times ``self_attention(..., rope=BASE)``:
the fused rotation (attention_rope.hip and the head dim 128 backward's epilogues) against the rotation in torch
around the fused kernels and around SDPA, and the rotation kernel alone.

With ``--head-dim 128 --window W`` (with or without ``--kv-heads``) it times ``self_attention(..., causal=True,
window=W)``: the band kernels of attention_d128.hip against the SDPA band-mask fallback and, at S <= 1024, the full
causal kernels, with the predicted ratio of block steps.

    python tools/bench_attention.py [calls] [--batch 128] [--seq 128] [--heads 12] [--lengths 0.5|random] [--causal]
                                    [--head-dim 64|128] [--kv-heads N] [--rope BASE] [--window W]"""
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


def sdpa_mask_fns(qkv, dout, NH, p, lengths):
    """(forward, backward) closures of BertLayer's mask path for the key mask of ``lengths``."""
    B, S, D3 = qkv.shape
    mask = (torch.arange(S, device=qkv.device).view(1, 1, 1, S) < lengths.view(B, 1, 1, 1))
    q = qkv.clone().requires_grad_(True)

    def fwd():
        qq, k, v = q.view(B, S, 3, NH, 64).permute(2, 0, 3, 1, 4)
        a = torch.nn.functional.scaled_dot_product_attention(qq, k, v, attn_mask=mask, dropout_p=p)
        return a.transpose(1, 2).reshape(B, S, NH * 64)

    y = fwd()
    return fwd, lambda: torch.autograd.grad(y, q, dout, retain_graph=True)


def padded(args, H, qkv, dout, scale):
    """Forward + backward time per variant on a padded batch, the variants alternating over the rounds."""
    B, S, NH = args.batch, args.seq, args.heads
    if args.lengths == "random":
        g = torch.Generator().manual_seed(args.seed)
        lengths = torch.randint(1, S + 1, (B,), generator=g, dtype=torch.int32).cuda()
    else:
        lengths = torch.full((B,), max(1, min(S, round(float(args.lengths) * S))), dtype=torch.int32, device="cuda")
    print("lengths %s: mean %.1f of %d tokens (%.0f %% valid)" % (
        args.lengths, lengths.float().mean().item(), S, 100 * lengths.float().mean().item() / S), flush=True)
    for p in (0.1, 0.0):
        out, lse = H.attention_forward(qkv, NH, scale, 1234, p)
        lout, llse = H.attention_forward(qkv, NH, scale, 1234, p, lengths=lengths)
        sf, sb = sdpa_mask_fns(qkv, dout, NH, p, lengths)
        full = (lambda: H.attention_forward(qkv, NH, scale, 1234, p),
                lambda: H.attention_backward(qkv, out, lse, dout, NH, scale, 1234, p))
        variants = {
            "full": full, "full again": full,
            "lengths": (lambda: H.attention_forward(qkv, NH, scale, 1234, p, lengths=lengths),
                        lambda: H.attention_backward(qkv, lout, llse, dout, NH, scale, 1234, p, lengths=lengths)),
            "sdpa mask": (sf, sb)}
        ts = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, (f, b) in variants.items():
                ts[k].append((med(f, args.calls), med(b, args.calls)))
        m = {}
        for k, v in ts.items():
            tot = sorted(f + b for f, b in v)
            m[k] = tot[len(tot) // 2]
            print("p=%.1f  %-10s fwd %7.1f us  bwd %7.1f us  fwd+bwd median %7.1f us (min %7.1f max %7.1f over %d rounds)" % (
                p, k, sorted(f for f, _ in v)[len(v) // 2], sorted(b for _, b in v)[len(v) // 2], m[k], tot[0], tot[-1],
                len(v)), flush=True)
        print("p=%.1f  full again / full %.3f   lengths / full %.3f   lengths / sdpa mask %.3f" % (
            p, m["full again"] / m["full"], m["lengths"] / m["full"], m["lengths"] / m["sdpa mask"]), flush=True)


def causal(args, H, qkv, dout, scale):
    """Forward and backward time per variant of a causal call, the variants alternating over the rounds."""
    B, S, NH = args.batch, args.seq, args.heads
    n = S // 64
    print("causal: block steps (n + 1) / 2n of the bidirectional call = %.3f" % ((n + 1) / (2 * n)), flush=True)
    for p in (0.1, 0.0):
        cout, clse = H.attention_forward(qkv, NH, scale, 1234, p, causal=True)
        q = qkv.clone().requires_grad_(True)

        def sdpa_fwd():
            qq, k, v = q.view(B, S, 3, NH, 64).permute(2, 0, 3, 1, 4)
            a = torch.nn.functional.scaled_dot_product_attention(qq, k, v, dropout_p=p, is_causal=True)
            return a.transpose(1, 2).reshape(B, S, NH * 64)

        y = sdpa_fwd()
        variants = {}
        for name, plain in (("causal", False), ("causal plain", True)):
            variants[name] = (
                lambda plain=plain: H.attention_forward(qkv, NH, scale, 1234, p, causal=True, plain_order=plain),
                lambda plain=plain: H.attention_backward(qkv, cout, clse, dout, NH, scale, 1234, p, causal=True,
                                                         plain_order=plain))
        if H.attention_supported(S, 64):  # the bidirectional kernels stop at S = 512
            out, lse = H.attention_forward(qkv, NH, scale, 1234, p)
            variants["full"] = variants["full again"] = (
                lambda: H.attention_forward(qkv, NH, scale, 1234, p),
                lambda: H.attention_backward(qkv, out, lse, dout, NH, scale, 1234, p))
        variants["sdpa causal"] = (sdpa_fwd, lambda: torch.autograd.grad(y, q, dout, retain_graph=True))
        ts = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, (f, b) in variants.items():
                ts[k].append((med(f, args.calls), med(b, args.calls)))
        m = {}
        for k, v in ts.items():
            fs, bs = sorted(f for f, _ in v), sorted(b for _, b in v)
            m[k] = (fs[len(fs) // 2], bs[len(bs) // 2])
            print("p=%.1f  %-12s fwd %7.1f us (min %7.1f max %7.1f)  bwd %7.1f us (min %7.1f max %7.1f) over %d rounds" % (
                p, k, m[k][0], fs[0], fs[-1], m[k][1], bs[0], bs[-1], len(v)), flush=True)
        for i, d in enumerate(("fwd", "bwd")):
            c = m["causal"][i]
            line = "p=%.1f  %s: causal / plain order %.3f   causal / sdpa causal %.3f" % (
                p, d, c / m["causal plain"][i], c / m["sdpa causal"][i])
            if "full" in m:
                line += "   causal / full %.3f   full again / full %.3f" % (c / m["full"][i], m["full again"][i] / m["full"][i])
            print(line, flush=True)


def d128(args, H, qkv, dout):
    """Head dim 128, multi-head: forward and backward time of the attention_d128.hip kernels (timed twice per round: ``d128
    again`` / ``d128`` is the run-to-run spread) and of the SDPA path with the permutes, the transposed output copy
    and the dq/dk/dv concatenation, the variants alternating over the rounds; bidirectional, or causal with --causal."""
    B, S, NH, c = args.batch, args.seq, args.heads, args.causal
    scale = 128 ** -0.5
    for p in (0.1, 0.0):
        out, lse = H.attention_d128_forward(qkv, NH, scale, 1234, p, c)
        q = qkv.clone().requires_grad_(True)

        def sdpa_fwd():
            qq, k, v = q.view(B, S, 3, NH, 128).permute(2, 0, 3, 1, 4)
            a = torch.nn.functional.scaled_dot_product_attention(qq, k, v, dropout_p=p, is_causal=c)
            return a.transpose(1, 2).reshape(B, S, NH * 128)

        y = sdpa_fwd()
        fused = (lambda: H.attention_d128_forward(qkv, NH, scale, 1234, p, c),
                 lambda: H.attention_d128_backward(qkv, out, lse, dout, NH, scale, 1234, p, c))
        variants = {"d128": fused, "d128 again": fused,
                    "sdpa": (sdpa_fwd, lambda: torch.autograd.grad(y, q, dout, retain_graph=True))}
        ts = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, (f, b) in variants.items():
                ts[k].append((med(f, args.calls), med(b, args.calls)))
        m = {}
        for k, v in ts.items():
            fs, bs, tot = sorted(f for f, _ in v), sorted(b for _, b in v), sorted(f + b for f, b in v)
            m[k] = tot[len(tot) // 2]
            print("causal=%d S=%d p=%.1f  %-10s fwd %7.1f us  bwd %7.1f us  fwd+bwd %7.1f us (min %7.1f max %7.1f) over %d rounds" % (
                c, S, p, k, fs[len(fs) // 2], bs[len(bs) // 2], m[k], tot[0], tot[-1], len(v)), flush=True)
        print("causal=%d S=%d p=%.1f  fwd+bwd: d128 / sdpa %.3f   d128 again / d128 %.3f" % (
            c, S, p, m["d128"] / m["sdpa"], m["d128 again"] / m["d128"]), flush=True)


def gqa(args, H):
    """Grouped-query heads at head dim 128 (``--kv-heads``): forward and backward time of the attention_d128.hip
    kernels (twice per round: ``gqa again`` / ``gqa`` is the run-to-run spread) against what serves the same call
    without grouping: ``expand`` (repeat_interleave of K/V into [B, S, 3*H*128], the same kernels at G = 1 on it, the
    torch group sum of the bf16 dk / dv slices and the concatenation into the grouped layout) and ``sdpa``
    (self_attention's fallback with ``_GQA_ENABLED = False``).  The variants alternate over the rounds."""
    B, S, NH, NKV, c = args.batch, args.seq, args.heads, args.kv_heads, args.causal
    G, scale = NH // NKV, 128 ** -0.5
    torch.manual_seed(0)
    qkv = (torch.randn(B, S, (NH + 2 * NKV) * 128, device="cuda") * 0.5).bfloat16()
    dout = (torch.randn(B, S, NH * 128, device="cuda") * 0.1).bfloat16()

    def expand():
        q, k, v = qkv.split((NH * 128, NKV * 128, NKV * 128), dim=2)
        k, v = (t.view(B, S, NKV, 128).repeat_interleave(G, dim=2).view(B, S, NH * 128) for t in (k, v))
        return torch.cat((q, k, v), dim=2)

    for p in (0.1, 0.0):
        out, lse = H.attention_gqa_forward(qkv, NH, NKV, scale, 1234, p, c)
        x = expand()
        xout, xlse = H.attention_d128_forward(x, NH, scale, 1234, p, c)
        assert torch.equal(out, xout)

        def expand_bwd():
            dx = H.attention_d128_backward(x, xout, xlse, dout, NH, scale, 1234, p, c).view(B, S, 3, NKV, G, 128)
            return torch.cat((dx[:, :, 0].reshape(B, S, NH * 128), dx[:, :, 1].sum(3).view(B, S, NKV * 128),
                              dx[:, :, 2].sum(3).view(B, S, NKV * 128)), dim=2)

        q = qkv.clone().requires_grad_(True)
        attn._GQA_ENABLED = False
        try:
            y = attn.self_attention(q, NH, p, causal=c, kv_heads=NKV)
        finally:
            attn._GQA_ENABLED = True
        assert type(y.grad_fn).__name__ != "_AttnGQAFnBackward"

        def sdpa_fwd():
            attn._GQA_ENABLED = False
            try:
                return attn.self_attention(q, NH, p, causal=c, kv_heads=NKV)
            finally:
                attn._GQA_ENABLED = True

        fused = (lambda: H.attention_gqa_forward(qkv, NH, NKV, scale, 1234, p, c),
                 lambda: H.attention_gqa_backward(qkv, out, lse, dout, NH, NKV, scale, 1234, p, c))
        variants = {"gqa": fused, "gqa again": fused,
                    "expand": (lambda: H.attention_d128_forward(expand(), NH, scale, 1234, p, c), expand_bwd),
                    "sdpa": (sdpa_fwd, lambda: torch.autograd.grad(y, q, dout, retain_graph=True))}
        ts = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, (f, b) in variants.items():
                ts[k].append((med(f, args.calls), med(b, args.calls)))
        m = {}
        for k, v in ts.items():
            fs, bs, tot = sorted(f for f, _ in v), sorted(b for _, b in v), sorted(f + b for f, b in v)
            m[k] = tot[len(tot) // 2]
            print("causal=%d S=%d B=%d G=%d p=%.1f  %-10s fwd %7.1f us  bwd %7.1f us  fwd+bwd %7.1f us (min %7.1f max %7.1f) over %d rounds" % (
                c, S, B, G, p, k, fs[len(fs) // 2], bs[len(bs) // 2], m[k], tot[0], tot[-1], len(v)), flush=True)
        print("causal=%d S=%d B=%d G=%d p=%.1f  fwd+bwd: gqa / expand %.3f   gqa / sdpa %.3f   gqa again / gqa %.3f" % (
            c, S, B, G, p, m["gqa"] / m["expand"], m["gqa"] / m["sdpa"], m["gqa again"] / m["gqa"]), flush=True)


def rope(args, H):
    """Rotary position embeddings at head dim 128 (``--rope BASE``, with or without ``--kv-heads``): forward and
    backward time of ``self_attention(..., rope=BASE)`` on its three routes, the variants alternating over the rounds:
    ``rope`` (attention_rope.hip, the head dim 128 forward on its result, the backward with the rotation in its
    epilogues; twice per round: ``rope again`` / ``rope`` is the run-to-run spread), ``torch+fused`` (``_ROPE_ENABLED =
    False``: Q and K rotated in torch around the fused kernels, autograd rotating dqkv back) and ``torch+sdpa`` (the
    fused attention switched off as well).  Then the rotation kernel alone with its bytes/s against a 5.3 TB/s
    streaming roofline."""
    B, S, NH, c, base = args.batch, args.seq, args.heads, args.causal, args.rope
    NKV = NH if args.kv_heads is None else args.kv_heads
    G, kv = NH // NKV, args.kv_heads
    torch.manual_seed(0)
    qkv = (torch.randn(B, S, (NH + 2 * NKV) * 128, device="cuda") * 0.5).bfloat16()
    dout = (torch.randn(B, S, NH * 128, device="cuda") * 0.1).bfloat16()
    cos, sin = attn.rope_tables(S, base, qkv.device)
    switches = {"rope": {}, "torch+fused": {"_ROPE_ENABLED": False},
                "torch+sdpa": {"_ROPE_ENABLED": False, "_GQA_ENABLED": False, "_D128_ENABLED": False}}
    fused_fns = ("_AttnRopeFnBackward", "_AttnGQAFnBackward", "_AttnD128FnBackward")

    def route(name, q, p):
        for k, v in switches[name].items():
            setattr(attn, k, v)
        try:
            return attn.self_attention(q, NH, p, causal=c, kv_heads=kv, rope=base)
        finally:
            for k in switches[name]:
                setattr(attn, k, True)

    tag = "causal=%d S=%d B=%d G=%d" % (c, S, B, G)
    for p in (0.1, 0.0):
        variants = {}
        for name in switches:
            q = qkv.clone().requires_grad_(True)
            y = route(name, q, p)
            assert (type(y.grad_fn).__name__ == fused_fns[0]) == (name == "rope"), (name, y.grad_fn)
            assert name != "torch+sdpa" or type(y.grad_fn).__name__ not in fused_fns, y.grad_fn
            variants[name] = (lambda name=name, q=q: route(name, q, p),
                              lambda y=y, q=q: torch.autograd.grad(y, q, dout, retain_graph=True))
        variants = {"rope": variants["rope"], "rope again": variants["rope"], "torch+fused": variants["torch+fused"],
                    "torch+sdpa": variants["torch+sdpa"]}
        ts = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, (f, b) in variants.items():
                ts[k].append((med(f, args.calls), med(b, args.calls)))
        m = {}
        for k, v in ts.items():
            fs, bs, tot = sorted(f for f, _ in v), sorted(b for _, b in v), sorted(f + b for f, b in v)
            m[k] = tot[len(tot) // 2]
            print("%s p=%.1f  %-11s fwd %7.1f us  bwd %7.1f us  fwd+bwd %7.1f us (min %7.1f max %7.1f) over %d rounds" % (
                tag, p, k, fs[len(fs) // 2], bs[len(bs) // 2], m[k], tot[0], tot[-1], len(v)), flush=True)
        print("%s p=%.1f  fwd+bwd: rope / torch+fused %.3f   rope / torch+sdpa %.3f   rope again / rope %.3f" % (
            tag, p, m["rope"] / m["torch+fused"], m["rope"] / m["torch+sdpa"], m["rope again"] / m["rope"]), flush=True)
    rs = sorted(med(lambda: H.rope_forward(qkv, NH, NKV, cos, sin), args.calls) for _ in range(args.rounds))
    t, nbytes = rs[len(rs) // 2], 2 * qkv.numel() * 2 + 2 * cos.numel() * 4  # qkv read and written once, the tables once
    print("%s rope_forward alone %7.1f us (min %7.1f max %7.1f): %.2f TB/s of %d bytes, %.0f %% of 5.3 TB/s" % (
        tag, t, rs[0], rs[-1], nbytes / t / 1e6, nbytes, 100 * nbytes / 5.3e6 / t), flush=True)


def window(args, H):
    """Sliding-window causal attention at head dim 128 (``--window W``, with or without ``--kv-heads``): forward and
    backward time of ``self_attention(..., causal=True, window=W)`` on the band kernels (twice per round: ``band
    again`` / ``band`` is the run-to-run spread), on its SDPA band-mask fallback (``_WINDOW_ENABLED = False``) and,
    where S <= 1024, of the full causal kernels at the same shape, next to the predicted ratio of block steps
    sum over qb of (min(qb, w) + 1) against n (n + 1) / 2.  The variants alternate over the rounds."""
    B, S, NH, W = args.batch, args.seq, args.heads, args.window
    NKV = NH if args.kv_heads is None else args.kv_heads
    G, kv, n, w = NH // NKV, args.kv_heads, S // 64, W // 64
    torch.manual_seed(0)
    qkv = (torch.randn(B, S, (NH + 2 * NKV) * 128, device="cuda") * 0.5).bfloat16()
    dout = (torch.randn(B, S, NH * 128, device="cuda") * 0.1).bfloat16()
    steps = sum(min(qb, w) + 1 for qb in range(n)) / (n * (n + 1) / 2)
    tag = "S=%d W=%d B=%d G=%d" % (S, W, B, G)

    def route(enabled, q, p, win):
        attn._WINDOW_ENABLED = enabled
        try:
            return attn.self_attention(q, NH, p, causal=True, kv_heads=kv, window=win)
        finally:
            attn._WINDOW_ENABLED = True

    for p in (0.1, 0.0):
        variants = {}
        for name, enabled, win in (("band", True, W), ("sdpa mask", False, W)) + ((("causal", True, None),) if S <= 1024 else ()):
            q = qkv.clone().requires_grad_(True)
            y = route(enabled, q, p, win)
            assert (type(y.grad_fn).__name__ == "_AttnWindowFnBackward") == (name == "band"), (name, y.grad_fn)
            variants[name] = (lambda enabled=enabled, q=q, win=win: route(enabled, q, p, win),
                              lambda y=y, q=q: torch.autograd.grad(y, q, dout, retain_graph=True))
        variants = {"band": variants["band"], "band again": variants["band"],
                    **{k: v for k, v in variants.items() if k != "band"}}
        ts = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, (f, b) in variants.items():
                ts[k].append((med(f, args.calls), med(b, args.calls)))
        m = {}
        for k, v in ts.items():
            fs, bs, tot = sorted(f for f, _ in v), sorted(b for _, b in v), sorted(f + b for f, b in v)
            m[k] = tot[len(tot) // 2]
            print("%s p=%.1f  %-10s fwd %8.1f us  bwd %8.1f us  fwd+bwd %8.1f us (min %8.1f max %8.1f) over %d rounds" % (
                tag, p, k, fs[len(fs) // 2], bs[len(bs) // 2], m[k], tot[0], tot[-1], len(v)), flush=True)
        line = "%s p=%.1f  fwd+bwd: band / sdpa mask %.3f   band again / band %.3f" % (
            tag, p, m["band"] / m["sdpa mask"], m["band again"] / m["band"])
        if "causal" in m:
            line += "   band / causal %.3f (block steps %.3f)" % (m["band"] / m["causal"], steps)
        print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("calls", nargs="?", type=int, default=20, help="calls to time")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--lengths", default=None, help="padded batch: a fraction of S in (0, 1], or 'random'")
    ap.add_argument("--causal", action="store_true", help="causal attention: the triangular kernels and what they replace")
    ap.add_argument("--rounds", type=int, default=5, help="--lengths / --causal: rounds the variants alternate over")
    ap.add_argument("--seed", type=int, default=0, help="--lengths random: seed of the lengths")
    ap.add_argument("--head-dim", type=int, choices=(64, 128), default=64,
                    help="128: the attention_d128.hip kernels against SDPA (with --causal: the causal ones)")
    ap.add_argument("--kv-heads", type=int, default=None,
                    help="grouped-query heads (needs --head-dim 128): the attention_d128.hip kernels on them against "
                         "the expanded-K/V path and SDPA")
    ap.add_argument("--rope", type=float, default=None, metavar="BASE",
                    help="rotary position embeddings of this base (needs --head-dim 128, with or without --kv-heads): "
                         "the fused rotation against the rotation in torch around the fused kernels and around SDPA")
    ap.add_argument("--window", type=int, default=None, metavar="W",
                    help="sliding-window causal attention over W keys (needs --head-dim 128, with or without "
                         "--kv-heads): the band kernels against the SDPA band-mask fallback and, at S <= 1024, the full "
                         "causal kernels")
    args = ap.parse_args()
    n = args.calls
    H = hip()
    B, S, NH = args.batch, args.seq, args.heads
    if args.window is not None:
        if args.head_dim != 128 or (args.kv_heads is not None and (args.kv_heads < 1 or NH % args.kv_heads)):
            ap.error("--window needs --head-dim 128 and, if given, --kv-heads a divisor of --heads")
        if args.window >= S and S <= 1024:
            ap.error("--window >= --seq <= 1024 is the causal call: nothing to compare")
        print("B=%d S=%d H=%d Hkv=%s window=%d" % (B, S, NH, args.kv_heads, args.window), flush=True)
        return window(args, H)
    if args.rope is not None:
        if args.head_dim != 128 or (args.kv_heads is not None and (args.kv_heads < 1 or NH % args.kv_heads)):
            ap.error("--rope needs --head-dim 128 and, if given, --kv-heads a divisor of --heads")
        print("B=%d S=%d H=%d Hkv=%s rope=%g" % (B, S, NH, args.kv_heads, args.rope), flush=True)
        return rope(args, H)
    if args.kv_heads is not None:
        if args.head_dim != 128 or args.kv_heads < 1 or NH % args.kv_heads:
            ap.error("--kv-heads needs --head-dim 128 and a divisor of --heads")
        print("B=%d S=%d H=%d Hkv=%d" % (B, S, NH, args.kv_heads), flush=True)
        return gqa(args, H)
    D = NH * args.head_dim
    torch.manual_seed(0)
    qkv = (torch.randn(B, S, 3 * D, device="cuda") * 0.5).bfloat16()
    dout = (torch.randn(B, S, D, device="cuda") * 0.1).bfloat16()
    scale = 64 ** -0.5
    print("B=%d S=%d H=%d" % (B, S, NH), flush=True)
    if args.head_dim == 128:
        return d128(args, H, qkv, dout)
    if args.causal:
        return causal(args, H, qkv, dout, scale)
    if args.lengths is not None:
        return padded(args, H, qkv, dout, scale)
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
