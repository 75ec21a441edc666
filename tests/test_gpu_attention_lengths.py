"""GPU tests of the length-aware streaming attention kernels (csrc/kernels/attention_lengths.hip).

Reference: the f32 composition of test_gpu_attention_long.py with the kernels' own dropout mask, a key mask (keys
>= L) and the output times the query-valid mask; its padded rows of out and dqkv are exact zeros, as the kernels'.

Bounds.  Whole tensors: the existing out 2e-2, dqkv 3e-2.  Per (sequence, head, 64-row block): a full
block meets the existing BLOCK_BOUND; a block with n < 64 valid rows is allowed 2 x the worst error of
the UNMASKED streaming kernels over the first n rows of a block against the same f32 reference
(PARTIAL_ERR: S in {128 streamed, 192, 512}, p in {0, 0.1}, this file's inputs, worst of two processes):
    n =  1   out 3.25e-3   dq 4.17e-3   dk 3.55e-3   dv 3.57e-3
    n = 17   out 2.52e-3   dq 2.92e-3   dk 2.85e-3   dv 3.37e-3
    n = 36   out 2.48e-3   dq 2.77e-3   dk 2.79e-3   dv 2.94e-3
    n = 44   out 2.47e-3   dq 2.70e-3   dk 2.66e-3   dv 2.85e-3
    n = 63   out 2.44e-3   dq 2.64e-3   dk 2.86e-3   dv 2.72e-3
The length-aware kernels on the cases below: n = 1 up to 3.58e-3, 1 < n < 64 up to 2.68e-3, full blocks 2.73e-3.
With a single valid key the softmax is exactly one-hot, dS = P o (dP - D) cancels and the reference dq / dk block is
exactly zero (so are out / dv where that probability is dropped): the kernels must give exactly zero too, 0 / 0 = 0.
"""
import functools

import pytest
import torch

from test_gpu_attention_long import BLOCK_BOUND, SCALE, SEED, _hip, _inputs, _l2, _maxrel

pytestmark = pytest.mark.gpu
needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

B, H = 2, 3
CASES = [(128, (128, 1)), (128, (65, 64)), (128, (0, 100)), (192, (192, 63)), (192, (129, 17)), (512, (300, 449)),
         (512, (512, 1))]
PARTIAL_ERR = {1: (3.25e-3, 4.17e-3, 3.55e-3, 3.57e-3), 17: (2.52e-3, 2.92e-3, 2.85e-3, 3.37e-3),
               36: (2.48e-3, 2.77e-3, 2.79e-3, 2.94e-3), 44: (2.47e-3, 2.70e-3, 2.66e-3, 2.85e-3),
               63: (2.44e-3, 2.64e-3, 2.86e-3, 2.72e-3)}  # n valid rows: (out, dq, dk, dv), module docstring


def _len(lengths):
    return torch.tensor(lengths, dtype=torch.int32, device="cuda")


def _run(qkv, gout, p, lengths=None, stream_kernel=False):
    out, lse = _hip().attention_forward(qkv, H, SCALE, SEED, p, stream_kernel=stream_kernel, lengths=lengths)
    return out, lse, _hip().attention_backward(qkv, out, lse, gout, H, SCALE, SEED, p, stream_kernel=stream_kernel,
                                               lengths=lengths)


def f32_attention(qkv, heads, p=0.0, lengths=None, seed=None):
    """The f32 composition: key mask, the kernels' dropout mask (when seed), rows >= L zeroed; [B, S, heads*64] f32.
    A sequence of length 0 keeps its scores unmasked (finite) and is zeroed by the row mask."""
    from kungfu_amd.ops import dropout_seed
    from kungfu_amd.ops.attention import dropout_keep

    Bq, S, _ = qkv.shape
    q, k, v = qkv.float().view(Bq, S, 3, heads, 64).permute(2, 0, 3, 1, 4)
    L = (torch.full((Bq,), S, device=qkv.device) if lengths is None else lengths).view(Bq, 1, 1, 1)
    ar = torch.arange(S, device=qkv.device)
    s = (q @ k.transpose(-1, -2) / 8.0).masked_fill(~((ar.view(1, 1, 1, S) < L) | (L == 0)), float("-inf"))
    P = torch.softmax(s, dim=-1)
    if seed is not None:
        P = P * dropout_keep(dropout_seed.effective(seed), Bq, heads, S, p, device=qkv.device) / (1 - p)
    return ((P @ v) * (ar.view(1, 1, S, 1) < L)).transpose(1, 2).reshape(Bq, S, heads * 64)


def block_errors(got, ref, S):
    """[B, S/64, H] relative L2 errors per (sequence, block, head) of [B, S, H*64] tensors; 0 / 0 = 0, x / 0 = inf."""
    d = (got.float() - ref.float()).view(B, S // 64, 64, H, 64).pow(2).sum((2, 4)).sqrt()
    r = ref.float().view(B, S // 64, 64, H, 64).pow(2).sum((2, 4)).sqrt()
    return torch.where(d == 0, d, d / r)


@functools.lru_cache(maxsize=None)
def _case(S, lengths, p):
    from kungfu_amd.ops import dropout_seed

    dropout_seed.base("cuda")
    qkv, gout = _inputs(S)
    pad = torch.arange(S, device="cuda").view(1, S) >= _len(lengths).view(B, 1)
    qkv[pad], gout[pad] = 1e4, 1e4  # padding is read where it shares a block with valid rows: large, finite, no effect
    out, lse, dqkv = _run(qkv, gout, p, _len(lengths))
    x = qkv.detach().float().requires_grad_(True)
    ref = f32_attention(x, H, p, _len(lengths), SEED)
    ref.backward(gout.float())
    return {"qkv": qkv, "gout": gout, "out": out, "lse": lse, "dqkv": dqkv, "ref": ref.detach(), "rgrad": x.grad}


@needs_gpu
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("S,lengths", CASES)
def test_lengths_match_fp32(S, lengths, p):
    """Whole tensors, per block (full: BLOCK_BOUND, partial: 2 x PARTIAL_ERR), exact zeros on every padded row."""
    c = _case(S, lengths, p)
    nvalid = (_len(lengths).view(B, 1) - 64 * torch.arange(S // 64, device="cuda")).clamp(0, 64)  # [B, S/64]
    pad = (torch.arange(S, device="cuda").view(1, S) >= _len(lengths).view(B, 1))
    g, r = c["dqkv"].view(B, S, 3, H * 64), c["rgrad"].view(B, S, 3, H * 64)
    pairs = [("out", c["out"], c["ref"])] + [(n, g[:, :, t], r[:, :, t]) for t, n in enumerate(("dq", "dk", "dv"))]
    whole = {k: (_l2(a, b), _maxrel(a, b)) for k, a, b in (("out", c["out"], c["ref"]), ("dqkv", c["dqkv"], c["rgrad"]))}
    print("lengths S=%d %s p=%g: %s" % (S, lengths, p, whole))
    fails = []
    for i, (name, got, ref) in enumerate(pairs):
        assert torch.isfinite(got.float()).all(), name
        assert (got[pad] == 0).all() and (ref[pad] == 0).all(), name + ": padded rows must be exactly zero"
        e = block_errors(got.contiguous(), ref.contiguous(), S).amax(2)  # [B, S/64]
        for n in sorted(set(nvalid.flatten().tolist()) - {0}):
            worst = e[nvalid == n].max().item()
            bound = BLOCK_BOUND[name] if n == 64 else 2.0 * PARTIAL_ERR[n][i]
            print("  %-3s n=%2d worst block %.3e (bound %.3e)" % (name, n, worst, bound))
            if not worst <= bound:
                fails.append((name, n, worst, bound))
    assert not fails, fails
    assert max(whole["out"]) < 2e-2 and max(whole["dqkv"]) < 3e-2, whole


@needs_gpu
@pytest.mark.parametrize("S", [128, 192, 512])
def test_full_lengths_are_bitwise_the_unmasked_call(S):
    """lengths == S everywhere: out, lse and dqkv bitwise the streaming kernels' without lengths (p = 0.1)."""
    qkv, gout = _inputs(S)
    for a, b in zip(_run(qkv, gout, 0.1, _len((S, S))), _run(qkv, gout, 0.1, stream_kernel=True)):
        assert torch.equal(a, b)


@needs_gpu
@pytest.mark.parametrize("S,L", [(512, 256), (320, 192)])
def test_block_aligned_lengths_are_bitwise_the_shorter_call(S, L):
    """Every length a multiple of 64 inside a longer S: the valid rows are bitwise the unmasked streaming kernels at
    S = L (same forward query block: 128 at 512 / 256, 64 at 320 / 192; p = 0.1): no skipped or extra block."""
    qkv, gout = _inputs(S)
    out, lse, dqkv = _run(qkv, gout, 0.1, _len((L, L)))
    o2, l2, d2 = _run(qkv[:, :L].contiguous(), gout[:, :L].contiguous(), 0.1)
    assert torch.equal(out[:, :L], o2) and torch.equal(lse[:, :, :L], l2) and torch.equal(dqkv[:, :L], d2)
    assert not out[:, L:].any() and not dqkv[:, L:].any() and torch.isinf(lse[:, :, L:]).all()


@needs_gpu
def test_every_element_written():
    """out and dqkv are allocated uninitialised: each is made to land on a just-freed NaN-filled block of a private
    pool (asserted), so an element the kernels leave out would stay NaN.  Lengths (0, 100) at S = 192."""
    c = _case(192, (0, 100), 0.0)
    lens = _len((0, 100))  # allocated outside the pool
    for like, call, want in (
            (c["out"], lambda: _hip().attention_forward(c["qkv"], H, SCALE, SEED, 0.0, lengths=lens)[0], c["out"]),
            (c["qkv"], lambda: _hip().attention_backward(c["qkv"], c["out"], c["lse"], c["gout"], H, SCALE, SEED, 0.0,
                                                         lengths=lens), c["dqkv"])):
        pool = torch.cuda.MemPool()
        with torch.cuda.use_mem_pool(pool):
            junk = torch.full_like(like, float("nan"))
            ptr = junk.data_ptr()
            del junk
            got = call()
        assert got.data_ptr() == ptr, "the result did not reuse the NaN-filled block"
        assert torch.isfinite(got.float()).all() and torch.equal(got, want)
        del got


@needs_gpu
def test_graph_replay_follows_lengths_overwritten_in_place():
    """Captured once, lengths overwritten in place before each replay: bitwise the eager result (S = 256, p = 0)."""
    qkv, gout = _inputs(256)
    lengths = _len((256, 256))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _run(qkv, gout, 0.0, lengths)  # warm up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = _run(qkv, gout, 0.0, lengths)
    for new in ((100, 0), (193, 64), (256, 255)):
        lengths.copy_(_len(new))
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(got, _run(qkv, gout, 0.0, _len(new))):
            assert torch.equal(a, b), new


@needs_gpu
def test_refusals_and_routing():
    from kungfu_amd.models.bert import BertLayer
    from kungfu_amd.ops.attention import self_attention

    hip = _hip()
    qkv = torch.randn(2, 256, 3 * 2 * 64, device="cuda").bfloat16().requires_grad_(True)
    for bad in (torch.ones(2, dtype=torch.int64, device="cuda"), torch.ones(3, dtype=torch.int32, device="cuda"),
                torch.ones(2, dtype=torch.int32), torch.ones(4, dtype=torch.int32, device="cuda")[::2]):
        with pytest.raises(RuntimeError, match=r"lengths must be a contiguous int32 \[B\] tensor"):
            hip.attention_forward(qkv.detach(), 2, SCALE, 1, 0.0, lengths=bad)
        with pytest.raises(ValueError, match=r"lengths must be a contiguous int32 \[B\] tensor"):
            self_attention(qkv, 2, 0.0, bad)
    short = torch.zeros(2, 64, 3 * 64, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match=r"S = 64 has no length-aware kernel"):
        hip.attention_forward(short, 1, SCALE, 1, 0.0, lengths=_len((64, 3)))
    assert self_attention(short.requires_grad_(True), 1, 0.0, _len((64, 3))).grad_fn is not None  # S = 64: the fallback
    with pytest.raises(ValueError, match="either mask or lengths"):
        BertLayer(128, 2, 512)(torch.zeros(2, 128, 128), mask=torch.ones(2, 1, 1, 128, dtype=torch.bool),
                               lengths=torch.ones(2, dtype=torch.int32))
    y = self_attention(qkv, 2, 0.0, _len((256, 9)))
    assert type(y.grad_fn).__name__ == "_AttnFnBackward", y.grad_fn


@needs_gpu
def test_bert_layers_with_lengths_match_f32_attention(monkeypatch):
    """Two BertLayers (d = 128, 2 heads, S = 256, eval, bf16), padded batch: output and input gradient on the valid
    rows (incoming gradient zero on padded rows) against the same layers on the f32 composition; no further from it
    than 1.5 x the SDPA mask path's distance + the margins of test_bert_layers_match_f32_attention (1e-3 / 0.02)."""
    from kungfu_amd.models import bert

    torch.manual_seed(5)
    layers = [bert.BertLayer(128, 2, 512, 0.1).cuda().eval().to(torch.bfloat16) for _ in range(2)]
    lengths = _len((200, 77))
    valid = (torch.arange(256, device="cuda").view(1, 256) < lengths.view(2, 1)).view(2, 256, 1)
    x = torch.randn(2, 256, 128, device="cuda").bfloat16()
    g = torch.randn(2, 256, 128, device="cuda").bfloat16() * valid
    used = []

    def traced(qkv, heads, p=0.0, lengths=None):
        y = bert_self_attention(qkv, heads, p, lengths)
        used.append(type(y.grad_fn).__name__)
        return y

    def run(**kw):
        xx = x.clone().requires_grad_(True)
        y = xx
        for layer in layers:
            y = layer(y, **kw)
        y.backward(g)
        return (y.detach().float() * valid), (xx.grad.float() * valid)

    bert_self_attention = bert.self_attention
    monkeypatch.setattr(bert, "self_attention", traced)
    y1, g1 = run(lengths=lengths)
    assert used == ["_AttnFnBackward"] * 2, used
    y0, g0 = run(mask=valid.view(2, 1, 1, 256))
    monkeypatch.setattr(bert, "self_attention", lambda q, h, p=0.0, lengths=None: f32_attention(q, h, p, lengths).to(q.dtype))
    yf, gf = run(lengths=lengths)
    print("BertLayer x 2 with lengths: out fused %.3e sdpa-mask %.3e; dx fused %.3e sdpa-mask %.3e" % (
        _l2(y1, yf), _l2(y0, yf), _l2(g1, gf), _l2(g0, gf)))
    assert _l2(y1, yf) <= 1.5 * _l2(y0, yf) + 1e-3
    assert _l2(g1, gf) <= 1.5 * _l2(g0, gf) + 0.02
