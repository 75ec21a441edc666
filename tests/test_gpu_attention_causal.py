"""GPU tests of the causal streaming attention kernels (csrc/kernels/attention_causal.hip): S = 64 .. 1024.

The reference is the f32 torch composition with the scores masked by triu(1) and the kernels' own dropout mask.
Bounds are those of test_gpu_attention_long.py: whole tensors (out 2e-2, dqkv 3e-2) and BLOCK_BOUND per
(sequence, head, 64-row block), block 0 -- all diagonal -- included.
"""
import functools

import pytest
import torch

from test_gpu_attention_lengths import block_errors
from test_gpu_attention_long import BLOCK_BOUND, SCALE, SEED, _hip, _inputs, _l2, _maxrel

pytestmark = pytest.mark.gpu
needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

B, H = 2, 3


def _run(qkv, gout, p):
    out, lse = _hip().attention_forward(qkv, H, SCALE, SEED, p, causal=True)
    return out, lse, _hip().attention_backward(qkv, out, lse, gout, H, SCALE, SEED, p, causal=True)


def f32_causal(qkv, heads, p=0.0, seed=None):
    """The f32 composition: keys > query masked to -inf, the kernels' dropout mask (when seed); [B, S, heads*64] f32."""
    from kungfu_amd.ops import dropout_seed
    from kungfu_amd.ops.attention import dropout_keep

    Bq, S, _ = qkv.shape
    q, k, v = qkv.float().view(Bq, S, 3, heads, 64).permute(2, 0, 3, 1, 4)
    future = torch.ones(S, S, dtype=torch.bool, device=qkv.device).triu(1)
    P = torch.softmax((q @ k.transpose(-1, -2) / 8.0).masked_fill(future, float("-inf")), dim=-1)
    if seed is not None:
        P = P * dropout_keep(dropout_seed.effective(seed), Bq, heads, S, p, device=qkv.device) / (1 - p)
    return (P @ v).transpose(1, 2).reshape(Bq, S, heads * 64)


@functools.lru_cache(maxsize=None)
def _case(S, p):
    from kungfu_amd.ops import dropout_seed

    dropout_seed.base("cuda")
    qkv, gout = _inputs(S)
    out, lse, dqkv = _run(qkv, gout, p)
    x = qkv.detach().float().requires_grad_(True)
    ref = f32_causal(x, H, p, SEED)
    ref.backward(gout.float())
    return {"qkv": qkv, "gout": gout, "out": out, "lse": lse, "dqkv": dqkv, "ref": ref.detach(), "rgrad": x.grad}


@needs_gpu
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("S", [64, 128, 192, 512, 1024])
def test_causal_matches_fp32(S, p):
    """Whole tensors, every (sequence, head, block) within BLOCK_BOUND, all finite, dq row 0 exactly zero (one
    visible key: the softmax is one-hot there)."""
    c = _case(S, p)
    g, r = c["dqkv"].view(B, S, 3, H * 64), c["rgrad"].view(B, S, 3, H * 64)
    whole = {k: (_l2(a, b), _maxrel(a, b)) for k, a, b in (("out", c["out"], c["ref"]), ("dqkv", c["dqkv"], c["rgrad"]))}
    print("causal S=%d p=%g: %s" % (S, p, whole))
    fails = []
    for name, got, ref in [("out", c["out"], c["ref"])] + [(n, g[:, :, t], r[:, :, t]) for t, n in enumerate(("dq", "dk", "dv"))]:
        assert torch.isfinite(got.float()).all(), name
        e = block_errors(got.contiguous(), ref.contiguous(), S).amax((0, 2))  # [S/64]
        print("  %-3s block 0 %.3e, worst block %.3e (bound %.3e)" % (name, e[0].item(), e.max().item(), BLOCK_BOUND[name]))
        if not e.max().item() <= BLOCK_BOUND[name]:
            fails.append((name, e.tolist()))
    assert not fails, fails
    assert max(whole["out"]) < 2e-2 and max(whole["dqkv"]) < 3e-2, whole
    assert not r[:, 0, 0].any() and not g[:, 0, 0].any()


@needs_gpu
@pytest.mark.parametrize("S,L", [(512, 192), (1024, 512), (128, 64)])
def test_prefix_is_bitwise_the_shorter_call(S, L):
    """No gradient into rows >= L: the first L rows of out, lse and dqkv are bitwise the causal call on qkv[:, :L]
    (p = 0.1) -- one skipped block, one extra block or a mask off by one would show."""
    qkv, gout = _inputs(S)
    gout[:, L:] = 0
    out, lse, dqkv = _run(qkv, gout, 0.1)
    o2, l2, d2 = _run(qkv[:, :L].contiguous(), gout[:, :L].contiguous(), 0.1)
    assert torch.equal(out[:, :L], o2) and torch.equal(lse[:, :, :L], l2) and torch.equal(dqkv[:, :L], d2)


@needs_gpu
def test_future_keys_cannot_leak():
    """S = 256, p = 0: K rows >= 130 overwritten with 1e4 and V rows >= 130 with NaN leave out[:, :130] bitwise
    unchanged and finite.

    Queries 128 and 129 share the diagonal key block 128 .. 191, and their wave's 16 keys 128 .. 143, with the NaN
    rows of V.  Their probabilities there are exactly 0, but 0 * NaN = NaN in any matrix product over those keys (the
    f32 composition P @ v gives NaN for every row of such an input), so the forward sums each wave's 16 x 16 diagonal
    triangle per (query, key) outside the MFMA and reads no V row beyond its queries."""
    c = _case(256, 0.0)
    x = c["qkv"].clone().view(B, 256, 3, H * 64)
    x[:, 130:, 1], x[:, 130:, 2] = 1e4, float("nan")
    out = _hip().attention_forward(x.view(B, 256, 3 * H * 64), H, SCALE, SEED, 0.0, causal=True)[0]
    bad = (~torch.isfinite(out[:, :130].float())).any(2).any(0).nonzero().flatten().tolist()
    x[:, 130:, 2] = c["qkv"].view(B, 256, 3, H * 64)[:, 130:, 2]
    konly = _hip().attention_forward(x.view(B, 256, 3 * H * 64), H, SCALE, SEED, 0.0, causal=True)[0]
    print("future keys: non-finite rows below 130: %s; rows < 128 bitwise unchanged: %s; K = 1e4 alone unchanged: %s" % (
        bad, torch.equal(out[:, :128], c["out"][:, :128]), torch.equal(konly[:, :130], c["out"][:, :130])))
    assert torch.isfinite(out[:, :130].float()).all()
    assert torch.equal(out[:, :130], c["out"][:, :130])


@needs_gpu
def test_every_element_written():
    """out and dqkv are allocated uninitialised: each is made to land on a just-freed NaN-filled block of a private
    pool (asserted), so an element the kernels leave out would stay NaN (S = 192)."""
    c = _case(192, 0.0)
    for like, call, want in (
            (c["out"], lambda: _hip().attention_forward(c["qkv"], H, SCALE, SEED, 0.0, causal=True)[0], c["out"]),
            (c["qkv"], lambda: _hip().attention_backward(c["qkv"], c["out"], c["lse"], c["gout"], H, SCALE, SEED, 0.0,
                                                         causal=True), c["dqkv"])):
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
def test_graph_replay_equals_eager():
    """Forward + backward captured once and replayed twice: bitwise the eager call (S = 256, p = 0.1; the binding
    calls leave the device seed word alone, so the effective seed is the same)."""
    c = _case(256, 0.1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _run(c["qkv"], c["gout"], 0.1)  # warm up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = _run(c["qkv"], c["gout"], 0.1)
    for _ in range(2):
        for t in got:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, c[k]) for a, k in zip(got, ("out", "lse", "dqkv")))


@needs_gpu
def test_refusals_and_routing():
    from kungfu_amd.models.bert import BertLayer
    from kungfu_amd.ops.attention import self_attention

    lens = torch.full((2,), 256, dtype=torch.int32, device="cuda")
    qkv = torch.randn(2, 256, 3 * 2 * 64, device="cuda").bfloat16().requires_grad_(True)
    with pytest.raises(RuntimeError, match="causal attention takes no lengths"):
        _hip().attention_forward(qkv.detach(), 2, SCALE, 1, 0.0, lengths=lens, causal=True)
    with pytest.raises(ValueError, match="causal attention takes no lengths"):
        self_attention(qkv, 2, 0.0, lens, causal=True)
    for S in (1088, 96):  # the fallback
        x = torch.randn(1, S, 3 * 64, device="cuda").bfloat16().requires_grad_(True)
        assert not _hip().attention_causal_supported(S)
        assert self_attention(x, 1, causal=True).grad_fn is not None
    assert type(self_attention(qkv, 2, causal=True).grad_fn).__name__ == "_AttnFnBackward"
    with pytest.raises(ValueError, match="causal takes neither mask nor lengths"):
        BertLayer(128, 2, 512)(torch.zeros(2, 128, 128), mask=torch.ones(2, 1, 1, 128, dtype=torch.bool), causal=True)


@needs_gpu
def test_gpt_matches_f32_attention(monkeypatch):
    """GPTLM (2 layers, d = 128, 2 heads, S = 256, bf16, eval): lm_loss and the embedding gradients with the fused
    causal attention against the same model on the f32 composition; no further from it than 1.5 x the SDPA is_causal
    path's distance + the margins of test_bert_layers_with_lengths_match_f32_attention (1e-3 / 0.02)."""
    from kungfu_amd.models import bert
    from kungfu_amd.models.gpt import GPTLM, lm_loss, synthetic_lm_batch
    from kungfu_amd.ops import attention as attn

    torch.manual_seed(5)
    model = GPTLM(vocab=1000, d=128, layers=2, heads=2, ffn=512, max_pos=256).cuda().eval().to(torch.bfloat16)
    ids = synthetic_lm_batch(2, 256, 1000, device="cuda")
    used = []

    def traced(qkv, heads, p=0.0, lengths=None, causal=False):
        y = attn.self_attention(qkv, heads, p, lengths, causal)
        used.append((causal, type(y.grad_fn).__name__))
        return y

    def run():
        model.zero_grad()
        loss = lm_loss(model, ids)
        loss.backward()
        return loss.item(), torch.cat([model.tok.weight.grad, model.pos.weight.grad]).float()

    monkeypatch.setattr(bert, "self_attention", traced)
    l1, g1 = run()
    assert used == [(True, "_AttnFnBackward")] * 2, used
    monkeypatch.setattr(attn, "_LONG_ENABLED", False)  # S = 256 leaves the fused path: SDPA is_causal
    l0, g0 = run()
    assert "_AttnFnBackward" not in [u[1] for u in used[2:]], used
    monkeypatch.setattr(bert, "self_attention", lambda q, h, p=0.0, causal=False: f32_causal(q, h).to(q.dtype))
    lf, gf = run()
    print("GPT x 2: loss fused %.6f sdpa %.6f f32 %.6f; grad fused %.3e sdpa %.3e" % (l1, l0, lf, _l2(g1, gf), _l2(g0, gf)))
    assert abs(l1 - lf) <= 1.5 * abs(l0 - lf) + 1e-3
    assert _l2(g1, gf) <= 1.5 * _l2(g0, gf) + 0.02
