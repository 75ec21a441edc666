"""GPU tests of the streaming attention kernels (csrc/kernels/attention_long.hip): S = 192 .. 512.

Relative L2 errors against an f32 torch composition that uses the kernels' own dropout mask
(ops.attention.dropout_keep), over whole tensors (the bounds of
test_gpu.py::test_fused_attention_matches_fp32) and per (sequence, head, 64-row block), so one
wrong block is not diluted by the others.

Per-block bound.  The worst per-block relative L2 error of the whole-sequence S = 128 kernels on
this recipe (B = 2, H = 3, p in {0, 0.1}; the dropout seed base differs per process, three runs) was
measured as
    out 2.63e-3   dq 3.89e-3   dk 4.20e-3   dv 2.50e-3
and the streaming kernels are allowed 2 x that (rows up to four times longer, and the running
maximum's rescale adds roundings).  Measured for them, worst over S in {192 .. 512}, both p and
two runs:
    out 2.44e-3   dq 2.80e-3   dk 2.70e-3   dv 2.82e-3
and on the running-max inputs (keys of one block scaled by 6, or block j by 1 + j; S = 256):
    out 1.69e-3   dq 3.27e-3   dk 3.44e-3   dv 3.67e-3
Those inputs make the softmax nearly one-hot, where dS = P o (dP - D) cancels: a D taken from the
saved bf16 output (the whole-sequence kernels: dq 1.08e-2 per block on such inputs at S = 128) would
miss the bound, which is why the streaming dQ kernel sums D from P and dP in f32.
"""
import functools
import math
import os
import subprocess
import sys

import pytest
import torch

from attention_long_cases import B, H, known_answer
from conftest import ROOT

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

SCALE = 1.0 / 8.0
SEED = 12345
LONG = (192, 256, 320, 384, 448, 512)
# worst per-block error of the S = 128 whole-sequence kernels (module docstring); the bound is 2 x
BLOCK_ERR_128 = {"out": 2.63e-3, "dq": 3.89e-3, "dk": 4.20e-3, "dv": 2.50e-3}
BLOCK_BOUND = {k: 2.0 * v for k, v in BLOCK_ERR_128.items()}


def _hip():
    from kungfu_amd._lib import hip

    return hip()


def _l2(a, r):
    return ((a.float() - r.float()).norm() / r.float().norm()).item()


def _maxrel(a, r):  # test_gpu.py's _rel
    return ((a.float() - r.float()).abs().max() / (r.float().abs().max() + 1e-12)).item()


def _block_err(a, r, S):
    """Worst relative L2 over (sequence, head, 64-row block) of [B, S, H*64] tensors."""
    d = (a.float() - r.float()).view(B, S // 64, 64, H, 64)
    rr = r.float().view(B, S // 64, 64, H, 64)
    return (d.pow(2).sum((2, 4)).sqrt() / rr.pow(2).sum((2, 4)).sqrt()).max().item()


def _reference(qkv, gout, S, p, seed):
    """out [B, S, H*64] and dqkv [B, S, 3*H*64] of the f32 composition with the kernels' mask."""
    from kungfu_amd.ops import dropout_seed
    from kungfu_amd.ops.attention import dropout_keep

    x = qkv.detach().float().requires_grad_(True)
    q, k, v = x.view(B, S, 3, H, 64).permute(2, 0, 3, 1, 4)
    P = torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1)
    keep = dropout_keep(dropout_seed.effective(seed), B, H, S, p, device="cuda")
    if p > 0:
        frac = keep.float().mean().item()
        assert abs(frac - (1 - p)) < 0.01, frac
    ref = ((P * keep / (1 - p)) @ v).transpose(1, 2).reshape(B, S, H * 64)
    ref.backward(gout.float())
    return ref.detach(), x.grad


def _run(qkv, gout, p, seed=SEED, stream_kernel=False):
    """(out, lse, dqkv) straight from the bindings."""
    hip = _hip()
    out, lse = hip.attention_forward(qkv, H, SCALE, seed, p, stream_kernel=stream_kernel)
    dqkv = hip.attention_backward(qkv, out, lse, gout, H, SCALE, seed, p, stream_kernel=stream_kernel)
    return out, lse, dqkv


def _errors(out, dqkv, ref, rgrad, S):
    """Whole-tensor and per-block errors, printed before anything asserts on them."""
    g, r = dqkv.view(B, S, 3, H * 64), rgrad.view(B, S, 3, H * 64)
    e = {"out": _l2(out, ref), "out_max": _maxrel(out, ref), "dqkv": _l2(dqkv, rgrad), "dqkv_max": _maxrel(dqkv, rgrad),
         "blk_out": _block_err(out, ref, S)}
    for t, n in enumerate(("dq", "dk", "dv")):
        e[n] = _l2(g[:, :, t], r[:, :, t])
        e["blk_" + n] = _block_err(g[:, :, t].contiguous(), r[:, :, t].contiguous(), S)
    return e


def _inputs(S, mod=None):
    torch.manual_seed(41)
    x = torch.randn(B, S, 3, H, 64, device="cuda") * 1.5
    if mod is not None:
        x[:, :, 1] *= mod.view(1, S, 1, 1)  # per-key scale of K
    qkv = x.view(B, S, 3 * H * 64).bfloat16().contiguous()
    gout = torch.randn(B, S, H * 64, device="cuda").bfloat16()
    return qkv, gout


@functools.lru_cache(maxsize=None)
def _case(S, p, stream_kernel=False):
    """One forward + backward at (S, p) with its reference and errors, shared by the tests below."""
    from kungfu_amd.ops import dropout_seed

    dropout_seed.base("cuda")
    qkv, gout = _inputs(S)
    out, lse, dqkv = _run(qkv, gout, p, stream_kernel=stream_kernel)
    ref, rgrad = _reference(qkv, gout, S, p, SEED)
    e = _errors(out, dqkv, ref, rgrad, S)
    print("attention S=%d p=%g stream=%s: %s" % (S, p, stream_kernel, " ".join("%s=%.3e" % kv for kv in e.items())))
    return {"qkv": qkv, "gout": gout, "out": out, "lse": lse, "dqkv": dqkv, "ref": ref, "rgrad": rgrad, "err": e}


def _assert_bounds(e):
    assert e["out"] < 2e-2 and e["out_max"] < 2e-2, e
    assert e["dqkv"] < 3e-2 and e["dqkv_max"] < 3e-2, e
    for n in ("dq", "dk", "dv"):
        assert e[n] < 2e-2, (n, e)
    for n in ("out", "dq", "dk", "dv"):
        assert e["blk_" + n] <= BLOCK_BOUND[n], (n, e)


@needs_gpu
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("S", [192, 256, 320, 384, 448, 512])
def test_streaming_attention_matches_fp32(S, p):
    """Forward and dq / dk / dv against the f32 composition with the same mask: whole-tensor bounds of
    test_fused_attention_matches_fp32, per-block bound 2 x the S = 128 kernels' (module docstring)."""
    _assert_bounds(_case(S, p)["err"])


@needs_gpu
def test_streaming_kernels_against_whole_sequence_kernels():
    """S = 128 on both kernel families, same inputs, seed and p = 0.1: lse agrees to 1e-5 and the
    streaming kernels are at most 2 x as far from the f32 reference as the whole-sequence ones."""
    old, new = _case(128, 0.1, False), _case(128, 0.1, True)
    assert (old["lse"] - new["lse"]).abs().max().item() <= 1e-5
    for n in ("out", "dq", "dk", "dv"):
        assert new["err"][n] <= 2.0 * old["err"][n], (n, new["err"], old["err"])
        assert new["err"]["blk_" + n] <= 2.0 * old["err"]["blk_" + n], (n, new["err"], old["err"])


@needs_gpu
@pytest.mark.parametrize("S", [256, 512])
def test_forward_known_answer_bit_exact(S):
    """All keys equal, integer Q / K / V: P = 1/S exactly, O = colsum(V) / S with an exact f32 sum, so
    the bf16 output is the round-to-nearest-even of the float64 value, bit for bit (the exactness of
    the expectation is checked on the CPU in test_attention_long_cases.py).  S is a power of two, so
    S * O = RNE_bf16(colsum V) exactly and that integer form is what assert_bits_equal compares."""
    from kungfu_amd.utils.numerics import assert_bits_equal

    qkv, vsum, score = known_answer(S)
    out, lse = _hip().attention_forward(qkv.cuda().bfloat16(), H, SCALE, SEED, 0.0)
    got = (out.float() * S).bfloat16().view(B, S, H, 64)
    assert torch.equal(got.float() / S, out.float().view(B, S, H, 64))  # the scaling lost nothing
    assert_bits_equal(got, vsum.view(B, 1, H, 64).expand(B, S, H, 64).contiguous(), "O * S", ties=True)
    assert (lse.double().cpu() - (score + math.log(S))).abs().max().item() <= 1e-5


@needs_gpu
@pytest.mark.parametrize("which", ["first", "last", "rising"])
def test_running_max_paths(which):
    """S = 256, p = 0: the keys of one 64-key block scaled by 6 so that every query's maximum lies
    there -- in the first block (the max never moves again), in the last (everything before is
    rescaled at the end) -- or block j scaled by 1 + j (the max moves at every step).  Bounds as
    test_streaming_attention_matches_fp32, whole tensors and per block."""
    S = 256
    blk = torch.arange(S, device="cuda") // 64
    mod = {"first": torch.where(blk == 0, 6.0, 1.0), "last": torch.where(blk == 3, 6.0, 1.0),
           "rising": 1.0 + blk.float()}[which]
    qkv, gout = _inputs(S, mod)
    out, lse, dqkv = _run(qkv, gout, 0.0)
    ref, rgrad = _reference(qkv, gout, S, 0.0, SEED)
    e = _errors(out, dqkv, ref, rgrad, S)
    print("running max %s: %s" % (which, " ".join("%s=%.3e" % kv for kv in e.items())))
    _assert_bounds(e)


@needs_gpu
def test_deterministic():
    """Two forward + backward calls on the same inputs: bitwise equal out, lse, dqkv (S = 384, p = 0.1)."""
    c = _case(384, 0.1)
    out, lse, dqkv = _run(c["qkv"], c["gout"], 0.1)
    assert torch.equal(out, c["out"]) and torch.equal(lse, c["lse"]) and torch.equal(dqkv, c["dqkv"])


@needs_gpu
def test_graph_replay_equals_eager():
    """Forward + backward captured in one torch.cuda.graph (one stream) and replayed twice: bitwise the
    eager result (S = 256, p = 0)."""
    c = _case(256, 0.0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _run(c["qkv"], c["gout"], 0.0)  # warm up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, lse, dqkv = _run(c["qkv"], c["gout"], 0.0)
    for _ in range(2):
        out.zero_(), lse.zero_(), dqkv.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, c["out"]) and torch.equal(lse, c["lse"]) and torch.equal(dqkv, c["dqkv"])


@needs_gpu
@pytest.mark.parametrize("S", [192, 320])
def test_every_gradient_element_written(S):
    """dqkv is allocated uninitialised.  The backward runs in a private memory pool whose only free block
    is a just-freed NaN-filled tensor of dqkv's size, so dqkv lands on NaNs (asserted) and every element
    the kernels leave out would stay NaN."""
    c = _case(S, 0.0)
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        junk = torch.full_like(c["qkv"], float("nan"))
        ptr = junk.data_ptr()
        del junk
        dqkv = _hip().attention_backward(c["qkv"], c["out"], c["lse"], c["gout"], H, SCALE, SEED, 0.0)
    assert dqkv.data_ptr() == ptr, "dqkv did not reuse the NaN-filled block"
    assert torch.isfinite(dqkv.float()).all()
    assert torch.equal(dqkv, c["dqkv"])
    del dqkv


@needs_gpu
def test_routing_and_refusals():
    hip = _hip()
    for S in (64, 128) + LONG:
        assert hip.attention_supported(S, 64), S
    for S in (0, 32, 96, 200, 576, 1024):
        assert not hip.attention_supported(S, 64), S
    assert not hip.attention_supported(256, 32)
    bad = torch.zeros(1, 576, 3 * 64, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match=r"64, 128, 192, 256, 320, 384, 448 or 512"):
        hip.attention_forward(bad, 1, SCALE, 1, 0.0)
    short = torch.zeros(1, 64, 3 * 64, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match=r"stream_kernel needs S >= 128"):  # no streaming kernel at S = 64
        hip.attention_forward(short, 1, SCALE, 1, 0.0, stream_kernel=True)
    from kungfu_amd.ops.attention import _AttnFn, self_attention

    qkv = torch.randn(1, 256, 3 * 2 * 64, device="cuda").bfloat16().requires_grad_(True)
    y = self_attention(qkv, 2)
    assert type(y.grad_fn).__name__ == _AttnFn.__name__ + "Backward", y.grad_fn


@needs_gpu
def test_knob_sends_long_sequences_to_sdpa():
    """KUNGFU_ATTN_LONG=0 in a fresh process: S = 256 leaves the fused path, S = 128 stays on it."""
    code = ("import torch\n"
            "from kungfu_amd.ops.attention import self_attention\n"
            "for S in (256, 128):\n"
            "    q = torch.randn(1, S, 3 * 2 * 64, device='cuda').bfloat16().requires_grad_(True)\n"
            "    print(S, type(self_attention(q, 2).grad_fn).__name__)\n")
    env = dict(os.environ, KUNGFU_ATTN_LONG="0", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = dict(l.split() for l in r.stdout.strip().splitlines())
    assert lines["256"] != "_AttnFnBackward" and lines["128"] == "_AttnFnBackward", r.stdout


@needs_gpu
def test_bert_layers_match_f32_attention(monkeypatch):
    """Two BertLayers (d = 128, 2 heads) at S = 256, eval, bf16: output and input gradient with the fused
    attention against the same layers whose attention is the f32 composition; no further from it than
    1.5 x the SDPA path's distance (+ 1e-3 / 0.02, test_vgg16_fused_stack_matches_layered's margins)."""
    from kungfu_amd.models import bert
    from kungfu_amd.models.bert import BertLayer
    from kungfu_amd.ops import attention as attn

    torch.manual_seed(5)
    layers = torch.nn.Sequential(BertLayer(128, 2, 512, 0.1), BertLayer(128, 2, 512, 0.1)).cuda().eval()
    layers.to(torch.bfloat16)  # LayerNorm too: rows of 128 run torch's layer_norm, which wants one dtype
    x = torch.randn(2, 256, 128, device="cuda").bfloat16()
    g = torch.randn(2, 256, 128, device="cuda").bfloat16()
    used = []

    def f32_attention(qkv, heads, p=0.0):
        Bq, S, _ = qkv.shape
        q, k, v = qkv.float().view(Bq, S, 3, heads, 64).permute(2, 0, 3, 1, 4)
        P = torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1)
        return (P @ v).transpose(1, 2).reshape(Bq, S, heads * 64).to(qkv.dtype)

    def traced(qkv, heads, p=0.0):
        y = attn.self_attention(qkv, heads, p)
        used.append(type(y.grad_fn).__name__)
        return y

    def run():
        xx = x.clone().requires_grad_(True)
        y = layers(xx)
        y.backward(g)
        return y.detach().float(), xx.grad.float()

    monkeypatch.setattr(bert, "self_attention", traced)
    y1, g1 = run()
    assert used == ["_AttnFnBackward"] * 2, used
    monkeypatch.setattr(attn, "_LONG_ENABLED", False)
    y0, g0 = run()
    assert "_AttnFnBackward" not in used[2:], used
    monkeypatch.setattr(bert, "self_attention", f32_attention)
    yf, gf = run()
    print("BertLayer x 2: out fused %.3e sdpa %.3e; dx fused %.3e sdpa %.3e" % (
        _l2(y1, yf), _l2(y0, yf), _l2(g1, gf), _l2(g0, gf)))
    assert _l2(y1, yf) <= 1.5 * _l2(y0, yf) + 1e-3
    assert _l2(g1, gf) <= 1.5 * _l2(g0, gf) + 0.02
