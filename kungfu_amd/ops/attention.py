"""Fused multi-head self-attention on the HIP kernels of csrc/kernels/attention.hip (S = 64 or
128: the whole sequence in LDS), csrc/kernels/attention_long.hip (S = 192 .. 512 in steps of
64: a resident row block, streamed column blocks, online softmax),
csrc/kernels/attention_lengths.hip (padded batches: the streaming kernels with per-sequence lengths) and
csrc/kernels/attention_causal.hip (causal: the streaming kernels with triangular trip counts, S up to 1024).

``self_attention(qkv, heads, p)`` takes the fused q/k/v projection output ``[B, S, 3*H*64]``
(the ``[B, S, 3, H, 64]`` layout of one ``nn.Linear(d, 3d)``) and returns the attention output
already in ``[B, S, H*64]`` (the layout the output projection consumes): no head permutes, no
transposed copies, and the backward writes dq/dk/dv straight into one ``[B, S, 3*H*64]``
gradient (no concatenation).  Dropout on the attention probabilities uses a counter hash of
(seed, b*H + h, query, key) -- the mask is recomputed in the backward, never stored;
:func:`dropout_keep` reproduces it in torch for the tests.

Padded batches: ``self_attention(qkv, heads, p, lengths)`` with ``lengths`` an int32 ``[B]`` tensor on
``qkv``'s device (values are clamped to [0, S]).  Sequence ``b`` attends to its first ``lengths[b]`` keys only;
its rows at or beyond that length come out exactly zero and receive exactly zero dq / dk / dv, and a length of 0
gives an all-zero sequence (no NaN).  S = 128 .. 512 runs the length-aware streaming kernels, whose block loops stop
at the length: padding costs nothing there.  ``lengths`` is read on the device only -- no host sync, and a
captured graph follows a ``lengths`` tensor overwritten in place.  The padded rows of ``qkv`` and of the
incoming gradient must be finite (they share 64-row blocks with valid rows).

Covers BERT's shapes (S a multiple of 64 up to 512 tokens, head dim 64; no general attention mask, only
per-sequence lengths); anything else runs ``F.scaled_dot_product_attention``, and so does S > 128 with
``KUNGFU_ATTN_LONG=0``.  With ``lengths`` the fallback (CPU, f32, S = 64, ``KUNGFU_ATTN_LONG=0``) is a torch
composition of the same semantics (:func:`_lengths_fallback`).

Causal (decoder) attention: ``self_attention(qkv, heads, p, causal=True)`` -- query ``q`` attends to keys ``k <= q``.
Every S that is a multiple of 64 from 64 to 1024 runs the triangular streaming kernels of
csrc/kernels/attention_causal.hip: query block ``i`` streams key blocks ``0 .. i`` only and just the diagonal block
is masked, so about half of the bidirectional call's work is never issued (profiles/attention_causal.md).  Same
layouts, same dropout hash, bitwise reproducible.  ``causal`` with ``lengths`` is a ``ValueError``: right padding
cannot influence a valid causal row, so masking the loss is enough.  The fallback (CPU, f32, any other S, and
S > 128 with ``KUNGFU_ATTN_LONG=0``) is ``F.scaled_dot_product_attention(..., is_causal=True)``.

Head dim 128 (GPT-3 from 6.7 B up, the LLaMA family): the head dim is ``qkv.shape[2] // (3 * heads)``, and at 128
``[B, S, 3*H*128]`` runs the kernels of csrc/kernels/attention_d128.hip, bidirectional or ``causal``, for every S that
is a multiple of 64 from 64 to 1024: 256-byte LDS rows, the wave's Q rows in registers, 8 accumulator tiles, scale
1 / sqrt(128), the same layouts, dropout hash and bitwise reproducibility (profiles/attention_d128.md).  They are one
family with the grouped-query kernels below: multi-head attention is their instance with one head per group.  There is no
``lengths`` support at this head dim: head dim 128 with ``lengths`` runs :func:`_lengths_fallback`, and any other S, a
CPU or f32 tensor, S > 128 with ``KUNGFU_ATTN_LONG=0`` and the (mask, S) pairs of ``_D128_ROUTED_AWAY`` run
``F.scaled_dot_product_attention``.  Other head dims always do.  The module switch ``_D128_ENABLED = False`` sends
every head dim 128 call to its fallback (for tests and measurements in one process).

Grouped-query attention (LLaMA-2 70B and later; one K/V head: multi-query attention):
``self_attention(qkv, heads, p, causal=..., kv_heads=Hkv)`` with ``heads % Hkv == 0`` takes ``[B, S, (H + 2*Hkv)*dh]``,
the output of one ``nn.Linear(d, (H + 2*Hkv)*dh)``: the H query heads, then the Hkv key heads, then the Hkv value
heads.  Query head ``h`` reads K/V head ``h // (H // Hkv)``; the result is ``[B, S, H*dh]`` and the gradient one tensor in
the input's layout.  ``kv_heads=None`` or ``kv_heads == heads`` is the call without the keyword, through the paths
above.  At head dim 128 the kernels of csrc/kernels/attention_d128.hip serve grouped heads on the domain of multi-head
attention (bf16, contiguous, S a multiple of 64 from 64 to 1024, either mask): K and V are never expanded, the G workgroups that
share a K/V head are dispatched next to each other, and the dK/dV kernel sums a group's query heads in its f32
registers and rounds once (profiles/attention_gqa.md).  The dropout hash stays keyed on the query head.  ``kv_heads``
with ``lengths`` is a ``ValueError``.  Everything else (CPU, f32, other S, head dim 64, S > 128 with
``KUNGFU_ATTN_LONG=0``, the (mask, S, G) triples of ``_GQA_ROUTED_AWAY``, ``_GQA_ENABLED = False``) expands K/V over the
group and runs ``F.scaled_dot_product_attention``; autograd sums the group's dk / dv.

Rotary position embeddings (LLaMA 1/2/3, Mistral, Qwen, GPT-NeoX): ``self_attention(..., rope=base)`` (for instance
``10000.0``) rotates every Q and K head by its position 0 .. S-1 before the scores, in the half-split ("rotate_half")
convention over the whole head: with ``theta_i = base ** (-i / (dh/2))``, ``c = cos(t * theta_i)`` and
``s = sin(t * theta_i)``, ``x'[i] = x[i]*c - x[i + dh/2]*s`` and ``x'[i + dh/2] = x[i + dh/2]*c + x[i]*s`` for
``i < dh/2``; V is untouched.  (Meta's interleaved convention, pairs ``(2i, 2i + 1)``, is this one under a fixed
permutation of the projection's output columns of each Q and K head; it is not implemented.)  ``cos`` and ``sin`` are
f32 ``[S, dh/2]`` tables computed once in float64 and cached (:func:`rope_tables`).  At head dim 128, with or without
``kv_heads``, on the domain of the grouped-query kernels (:func:`eligible_gqa` for ``kv_heads or heads``; multi-head
attention runs them at G = 1, as it does without ``rope``) one streaming kernel
(csrc/kernels/attention_rope.hip) writes the rotated ``qkv`` once, in f32 with one rounding; the attention forward
reads it and it is what the backward keeps.  The gradient's transposed rotation runs in f32 in the epilogues of the dQ
and dK/dV kernels, ahead of their single rounding to bf16, so the backward has no pass over ``dqkv`` at all
(profiles/attention_rope.md).  Every other call (CPU, f32, head dim 64, other S, ``lengths``, ``_ROPE_ENABLED = False``,
the (mask, S, G) triples of ``_ROPE_ROUTED_AWAY``) rotates Q and K in torch, which autograd differentiates, and runs
``self_attention`` on the result without ``rope``: every path above is reached that way.  A ``rope`` that is not
positive and finite is a ``ValueError``; ``rope=None`` is the call without the keyword.

Sliding-window (local) causal attention (Mistral): ``self_attention(..., causal=True, window=W)`` -- query ``q`` attends
to keys ``q - W < k <= q``, at most ``W`` keys, itself included.  ``W`` is a positive multiple of 64.  At head dim 128,
with or without ``kv_heads`` and ``rope``, the band instantiations of csrc/kernels/attention_d128.hip's causal kernels
serve every S that is a multiple of 64 from 64 to 8192: query block ``i`` streams key blocks ``max(0, i - W/64) .. i``
only, the block at the band's lower edge and the diagonal block are the two masked ones, and the dK/dV kernel streams
the ``W/64 + 1`` query blocks that see its key block, so the work grows with ``S * W``, not ``S * S``
(profiles/attention_window.md).  Same layouts, dropout hash, rope epilogues and bitwise reproducibility; multi-head
attention runs them at one head per group.  ``W >= S`` is plain causal attention: for S <= 1024 it is the call without
``window`` (bitwise), beyond that the band kernels compute it, which makes ``window=S`` the long-context causal call.
``window`` without ``causal=True``, with ``lengths``, or not a positive multiple of 64 is a ``ValueError``;
``window=None`` is the call without the keyword.  Every other call (CPU, f32, head dim 64, other S, S > 128 with
``KUNGFU_ATTN_LONG=0``, ``_WINDOW_ENABLED = False``, ``rope`` with ``_ROPE_ENABLED = False``, the (S, W, G) triples of
``_WINDOW_ROUTED_AWAY``) rotates in torch if ``rope`` is given, expands K/V over the group and runs
``F.scaled_dot_product_attention`` with a boolean ``[S, S]`` band mask.
"""
from __future__ import annotations

import functools
import math
import os

import torch
import torch.nn.functional as F

from .._lib import hip, hip_available
from . import dropout_seed

# (round 6: the qkv bias gradient from column sums inside the attention backward is gone -- measured slower
# end to end than the projection's own two-stage column sum, BERT-base + GNS 15.70-15.76 -> 15.78-15.80
# ms/step on one box, r5t38)


# 0: sequences longer than 128 tokens go back to F.scaled_dot_product_attention
_LONG_ENABLED = os.environ.get("KUNGFU_ATTN_LONG", "1") != "0"


class _AttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, heads, p, seed, lengths=None, causal=False):
        scale = 1.0 / math.sqrt(64.0)
        if causal:  # (the keyword is passed only here: calls without it stay what they were)
            out, lse = hip().attention_forward(qkv, heads, scale, seed, p, causal=True)
        else:
            out, lse = hip().attention_forward(qkv, heads, scale, seed, p, lengths=lengths)
        ctx.save_for_backward(qkv, out, lse, lengths)  # lse is +inf on the padded rows: the backward's row mask
        ctx.heads, ctx.p, ctx.seed, ctx.scale, ctx.causal = heads, p, seed, scale, causal
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse, lengths = ctx.saved_tensors
        kw = dict(causal=True) if ctx.causal else dict(lengths=lengths)
        dqkv = hip().attention_backward(qkv, out, lse, dout.contiguous(), ctx.heads, ctx.scale, ctx.seed, ctx.p, **kw)
        return dqkv, None, None, None, None, None


class _AttnD128Fn(torch.autograd.Function):
    """Head dim 128, multi-head: the kernels of attention_d128.hip with one head per group."""

    @staticmethod
    def forward(ctx, qkv, heads, p, seed, causal):
        scale = 1.0 / math.sqrt(128.0)
        out, lse = hip().attention_d128_forward(qkv, heads, scale, seed, p, causal)
        ctx.save_for_backward(qkv, out, lse)
        ctx.heads, ctx.p, ctx.seed, ctx.scale, ctx.causal = heads, p, seed, scale, causal
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        dqkv = hip().attention_d128_backward(qkv, out, lse, dout.contiguous(), ctx.heads, ctx.scale, ctx.seed, ctx.p,
                                             ctx.causal)
        return dqkv, None, None, None, None


# (causal, S) pairs at head dim 128 whose forward + backward did not beat the SDPA path by more than the measured
# spread (profiles/attention_d128.md): they keep the fallback
_D128_ROUTED_AWAY: frozenset = frozenset()
# False: every head dim 128 call keeps its fallback, whatever S (KUNGFU_ATTN_LONG=0 leaves S <= 128 fused); tests and
# tools/bench_attention.py set it to compare the two paths in one process
_D128_ENABLED = True


def eligible_d128(qkv: torch.Tensor, heads: int, lengths=None, causal: bool = False) -> bool:
    """Whether the head dim 128 kernels serve this call: bf16, contiguous, on the GPU, S a multiple of 64 up to 1024
    that the measurements did not route away, no ``lengths``; ``KUNGFU_ATTN_LONG=0`` keeps S > 128 off them."""
    return (_D128_ENABLED and lengths is None and qkv.is_cuda and qkv.dtype == torch.bfloat16 and qkv.dim() == 3
            and qkv.is_contiguous() and qkv.shape[2] == 3 * heads * 128 and qkv.shape[1] <= 1024
            and (_LONG_ENABLED or qkv.shape[1] <= 128) and (bool(causal), int(qkv.shape[1])) not in _D128_ROUTED_AWAY
            and hip_available() and hip().attention_d128_supported(int(qkv.shape[1])))


class _AttnGQAFn(torch.autograd.Function):
    """Grouped-query heads at head dim 128: the kernels of attention_d128.hip."""

    @staticmethod
    def forward(ctx, qkv, heads, kv_heads, p, seed, causal):
        scale = 1.0 / math.sqrt(128.0)
        out, lse = hip().attention_gqa_forward(qkv, heads, kv_heads, scale, seed, p, causal)
        ctx.save_for_backward(qkv, out, lse)
        ctx.heads, ctx.kv_heads, ctx.p, ctx.seed, ctx.scale, ctx.causal = heads, kv_heads, p, seed, scale, causal
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        dqkv = hip().attention_gqa_backward(qkv, out, lse, dout.contiguous(), ctx.heads, ctx.kv_heads, ctx.scale,
                                            ctx.seed, ctx.p, ctx.causal)
        return dqkv, None, None, None, None, None


# (causal, S, G) triples whose forward + backward did not beat the better of the two alternatives (K/V expanded for the
# head dim 128 kernels plus the group sum; the SDPA fallback) by more than the measured spread
# (profiles/attention_gqa.md): they keep the fallback
_GQA_ROUTED_AWAY: frozenset = frozenset()
# False: every kv_heads call keeps its fallback (tests and tools/bench_attention.py compare the paths in one process)
_GQA_ENABLED = True


def eligible_gqa(qkv: torch.Tensor, heads: int, kv_heads: int, causal: bool = False) -> bool:
    """Whether the grouped-query kernels serve this call: head dim 128, bf16, contiguous, on the GPU, S a multiple of
    64 up to 1024 that the measurements did not route away; ``KUNGFU_ATTN_LONG=0`` keeps S > 128 off them."""
    return (_GQA_ENABLED and qkv.is_cuda and qkv.dtype == torch.bfloat16 and qkv.dim() == 3 and qkv.is_contiguous()
            and qkv.shape[2] == (heads + 2 * kv_heads) * 128 and qkv.shape[1] <= 1024
            and (_LONG_ENABLED or qkv.shape[1] <= 128)
            and (bool(causal), int(qkv.shape[1]), heads // kv_heads) not in _GQA_ROUTED_AWAY
            and hip_available() and hip().attention_gqa_supported(int(qkv.shape[1]), heads, kv_heads))


def _gqa_attention(qkv: torch.Tensor, heads: int, kv_heads: int, p: float, causal: bool) -> torch.Tensor:
    """``self_attention`` with ``kv_heads < heads``: the fused kernels, else K/V expanded over the group for SDPA."""
    B, S, W = qkv.shape
    if W % (heads + 2 * kv_heads):
        raise ValueError("self_attention: qkv's last dim %d is not (heads + 2*kv_heads) * dh for heads %d, kv_heads %d"
                         % (W, heads, kv_heads))
    if eligible_gqa(qkv, heads, kv_heads, causal):
        seed = int(torch.randint(0, 2**31 - 1, (1,)).item())  # CPU generator: no device sync
        dropout_seed.base(qkv.device)
        return _AttnGQAFn.apply(qkv, heads, kv_heads, float(p), seed, bool(causal))
    dh, G = W // (heads + 2 * kv_heads), heads // kv_heads
    q, k, v = qkv.split((heads * dh, kv_heads * dh, kv_heads * dh), dim=2)
    q = q.view(B, S, heads, dh).transpose(1, 2)
    k, v = (t.view(B, S, kv_heads, dh).transpose(1, 2).repeat_interleave(G, dim=1) for t in (k, v))
    a = F.scaled_dot_product_attention(q, k, v, dropout_p=p, is_causal=causal)
    return a.transpose(1, 2).reshape(B, S, heads * dh)


@functools.lru_cache(maxsize=None)
def _rope_tables(S: int, base: float, device: torch.device, half: int):
    theta = base ** (-torch.arange(half, dtype=torch.float64) / half)
    angle = torch.arange(S, dtype=torch.float64)[:, None] * theta[None]
    return angle.cos().float().to(device).contiguous(), angle.sin().float().to(device).contiguous()


def rope_tables(S: int, base: float, device, half: int = 64):
    """``(cos, sin)``, f32 ``[S, half]`` on ``device``: ``cos(t * base ** (-i / half))`` for position ``t`` and pair
    ``i``, evaluated in float64 (the angles reach S - 1 rad) and cached per (S, base, device, half).  The tables are
    shared between calls: do not write to them."""
    return _rope_tables(int(S), float(base), torch.device(device), int(half))


class _AttnRopeFn(torch.autograd.Function):
    """Rotary position embeddings at head dim 128: attention_rope.hip's rotation, then the kernels of
    attention_d128.hip on its result, whose backward rotates dq and dk back in its epilogues."""

    @staticmethod
    def forward(ctx, qkv, heads, kv_heads, p, seed, causal, base):
        scale = 1.0 / math.sqrt(128.0)
        cos, sin = rope_tables(qkv.shape[1], base, qkv.device)
        rot = hip().rope_forward(qkv, heads, kv_heads, cos, sin)
        out, lse = hip().attention_gqa_forward(rot, heads, kv_heads, scale, seed, p, causal)
        ctx.save_for_backward(rot, out, lse, cos, sin)  # the unrotated qkv is not kept
        ctx.heads, ctx.kv_heads, ctx.p, ctx.seed, ctx.scale, ctx.causal = heads, kv_heads, p, seed, scale, causal
        return out

    @staticmethod
    def backward(ctx, dout):
        rot, out, lse, cos, sin = ctx.saved_tensors
        dqkv = hip().attention_gqa_backward(rot, out, lse, dout.contiguous(), ctx.heads, ctx.kv_heads, ctx.scale,
                                            ctx.seed, ctx.p, ctx.causal, cos=cos, sin=sin)
        return dqkv, None, None, None, None, None, None


# (causal, S, G) triples whose forward + backward with the fused rotation did not beat the better of the rotation
# composed in torch around the fused kernels and around the SDPA path by more than the measured spread
# (profiles/attention_rope.md): they keep the fallback
_ROPE_ROUTED_AWAY: frozenset = frozenset()
# False: every rope call rotates in torch (tests and tools/bench_attention.py compare the paths in one process)
_ROPE_ENABLED = True


def _check_rope(qkv: torch.Tensor, heads: int, kv_heads, rope) -> int:
    """The ``ValueError``s of ``rope`` -> the number of K/V heads."""
    if isinstance(rope, bool) or not isinstance(rope, (int, float)) or not (0.0 < rope < math.inf):
        raise ValueError("self_attention: rope must be a positive finite base (for instance 10000.0), got %r" % (rope,))
    Hkv = heads if kv_heads is None else kv_heads
    W = qkv.shape[2]
    if Hkv < 1 or heads % Hkv or W % (2 * (heads + 2 * Hkv)):
        raise ValueError("self_attention: rope needs kv_heads to divide heads and qkv's last dim to be "
                         "(heads + 2*kv_heads) * dh with dh even, got %d for heads %d, kv_heads %d" % (W, heads, Hkv))
    return Hkv


def _rope_in_torch(qkv: torch.Tensor, heads: int, Hkv: int, rope: float) -> torch.Tensor:
    """``qkv`` with its Q and K heads rotated by torch operations, which autograd differentiates."""
    B, S, W = qkv.shape
    dh = W // (heads + 2 * Hkv)
    cos, sin = (t[None, :, None, :] for t in rope_tables(S, rope, qkv.device, dh // 2))
    x = qkv.view(B, S, heads + 2 * Hkv, dh)
    qk, v = x[:, :, :heads + Hkv], x[:, :, heads + Hkv:]
    # in f32 (f64 for f64 inputs) with one rounding, as the kernel
    x1, x2 = qk.to(torch.promote_types(qkv.dtype, torch.float32)).split(dh // 2, dim=3)
    rot = torch.cat((x1 * cos - x2 * sin, x2 * cos + x1 * sin), dim=3).to(qkv.dtype)
    return torch.cat((rot, v), dim=2).view(B, S, W)


def _rope_attention(qkv: torch.Tensor, heads: int, p: float, lengths, causal: bool, kv_heads, rope) -> torch.Tensor:
    """``self_attention`` with ``rope``: the fused rotation where the grouped-query kernels serve the call, else the
    rotation in torch around ``self_attention`` without ``rope``."""
    Hkv = _check_rope(qkv, heads, kv_heads, rope)
    B, S, W = qkv.shape
    if (_ROPE_ENABLED and lengths is None and W == (heads + 2 * Hkv) * 128 and eligible_gqa(qkv, heads, Hkv, causal)
            and (bool(causal), S, heads // Hkv) not in _ROPE_ROUTED_AWAY):
        seed = int(torch.randint(0, 2**31 - 1, (1,)).item())  # CPU generator: no device sync
        dropout_seed.base(qkv.device)
        return _AttnRopeFn.apply(qkv, heads, Hkv, float(p), seed, bool(causal), float(rope))
    return self_attention(_rope_in_torch(qkv, heads, Hkv, rope), heads, p, lengths, causal, kv_heads)


class _AttnWindowFn(torch.autograd.Function):
    """Sliding-window causal attention at head dim 128: the band instantiations of attention_d128.hip's causal kernels,
    behind attention_rope.hip's rotation when ``base`` is given (then the backward's epilogues rotate dq and dk back)."""

    @staticmethod
    def forward(ctx, qkv, heads, kv_heads, p, seed, window, base):
        scale = 1.0 / math.sqrt(128.0)
        cos, sin = (None, None) if base is None else rope_tables(qkv.shape[1], base, qkv.device)
        rot = qkv if base is None else hip().rope_forward(qkv, heads, kv_heads, cos, sin)
        out, lse = hip().attention_gqa_forward(rot, heads, kv_heads, scale, seed, p, True, window)
        ctx.save_for_backward(rot, out, lse, cos, sin)  # (with base the unrotated qkv is not kept)
        ctx.heads, ctx.kv_heads, ctx.p, ctx.seed, ctx.scale, ctx.window = heads, kv_heads, p, seed, scale, window
        return out

    @staticmethod
    def backward(ctx, dout):
        rot, out, lse, cos, sin = ctx.saved_tensors
        dqkv = hip().attention_gqa_backward(rot, out, lse, dout.contiguous(), ctx.heads, ctx.kv_heads, ctx.scale,
                                            ctx.seed, ctx.p, True, cos=cos, sin=sin, window=ctx.window)
        return dqkv, None, None, None, None, None, None


# (S, W, G) triples whose forward + backward on the band kernels did not beat the SDPA band-mask fallback by more than
# the measured spread (profiles/attention_window.md): they keep the fallback
_WINDOW_ROUTED_AWAY: frozenset = frozenset()
# False: every window call keeps its fallback (tests and tools/bench_attention.py compare the paths in one process)
_WINDOW_ENABLED = True


def eligible_window(qkv: torch.Tensor, heads: int, kv_heads: int, window: int) -> bool:
    """Whether the band kernels serve this causal call: head dim 128, bf16, contiguous, on the GPU, S a multiple of 64
    up to 8192 that the measurements did not route away; ``KUNGFU_ATTN_LONG=0`` keeps S > 128 off them."""
    return (_WINDOW_ENABLED and qkv.is_cuda and qkv.dtype == torch.bfloat16 and qkv.dim() == 3 and qkv.is_contiguous()
            and qkv.shape[2] == (heads + 2 * kv_heads) * 128 and qkv.shape[1] <= 8192
            and (_LONG_ENABLED or qkv.shape[1] <= 128)
            and (int(qkv.shape[1]), int(window), heads // kv_heads) not in _WINDOW_ROUTED_AWAY
            and hip_available() and hip().attention_gqa_supported(int(qkv.shape[1]), heads, kv_heads, int(window)))


def _window_attention(qkv: torch.Tensor, heads: int, p: float, lengths, causal: bool, kv_heads, rope,
                      window) -> torch.Tensor:
    """``self_attention`` with ``window``: the band kernels, else the rotation in torch (with ``rope``), K/V expanded
    over the group and SDPA with a boolean band mask."""
    if isinstance(window, bool) or not isinstance(window, int) or window <= 0 or window % 64:
        raise ValueError("self_attention: window must be a positive multiple of 64, got %r" % (window,))
    if not causal:
        raise ValueError("self_attention: window needs causal=True (query q attends to keys q - window < k <= q)")
    if lengths is not None:
        raise ValueError("self_attention: window takes no lengths")
    B, S, W = qkv.shape
    if window >= S and S <= 1024:  # plain causal attention on today's paths
        return self_attention(qkv, heads, p, None, True, kv_heads, rope)
    Hkv = heads if kv_heads is None else kv_heads
    if rope is not None:
        _check_rope(qkv, heads, kv_heads, rope)
    if Hkv < 1 or heads % Hkv or W % (heads + 2 * Hkv):
        raise ValueError("self_attention: kv_heads must divide heads and qkv's last dim must be (heads + 2*kv_heads) "
                         "* dh, got %d for heads %d, kv_heads %d" % (W, heads, Hkv))
    if eligible_window(qkv, heads, Hkv, window) and (rope is None or _ROPE_ENABLED):
        seed = int(torch.randint(0, 2**31 - 1, (1,)).item())  # CPU generator: no device sync
        dropout_seed.base(qkv.device)
        return _AttnWindowFn.apply(qkv, heads, Hkv, float(p), seed, int(window), None if rope is None else float(rope))
    if rope is not None:
        qkv = _rope_in_torch(qkv, heads, Hkv, rope)
    dh, G = W // (heads + 2 * Hkv), heads // Hkv
    q, k, v = qkv.split((heads * dh, Hkv * dh, Hkv * dh), dim=2)
    q = q.view(B, S, heads, dh).transpose(1, 2)
    k, v = (t.view(B, S, Hkv, dh).transpose(1, 2).repeat_interleave(G, dim=1) for t in (k, v))
    pos = torch.arange(S, device=qkv.device)
    band = (pos[None, :] <= pos[:, None]) & (pos[None, :] > pos[:, None] - window)  # [query, key]
    a = F.scaled_dot_product_attention(q, k, v, attn_mask=band, dropout_p=p)
    return a.transpose(1, 2).reshape(B, S, heads * dh)


def eligible(qkv: torch.Tensor, heads: int, lengths=None, causal: bool = False) -> bool:
    """Whether the fused kernels serve this call; with ``lengths`` only the streaming family does
    (S >= 128, and not with ``KUNGFU_ATTN_LONG=0``); ``causal``: S a multiple of 64 up to 1024, no lengths."""
    if causal:
        return (lengths is None and qkv.is_cuda and qkv.dtype == torch.bfloat16 and qkv.dim() == 3
                and qkv.is_contiguous() and qkv.shape[2] == 3 * heads * 64 and qkv.shape[1] <= 1024
                and (_LONG_ENABLED or qkv.shape[1] <= 128)
                and hip_available() and hip().attention_causal_supported(int(qkv.shape[1])))
    return (qkv.is_cuda and qkv.dtype == torch.bfloat16 and qkv.dim() == 3 and qkv.is_contiguous()
            and qkv.shape[2] == 3 * heads * 64 and (_LONG_ENABLED or qkv.shape[1] <= 128)
            and (lengths is None or (_LONG_ENABLED and qkv.shape[1] >= 128))
            and hip_available() and hip().attention_supported(int(qkv.shape[1]), 64))


def _check_lengths(qkv: torch.Tensor, lengths: torch.Tensor) -> None:
    if (lengths.dtype != torch.int32 or lengths.shape != (qkv.shape[0],) or lengths.device != qkv.device
            or not lengths.is_contiguous()):
        raise ValueError("self_attention: lengths must be a contiguous int32 [B] tensor on qkv's device, got %s %s "
                         "(strides %s) on %s" % (lengths.dtype, tuple(lengths.shape), lengths.stride(), lengths.device))


def _lengths_fallback(qkv: torch.Tensor, heads: int, p: float, lengths: torch.Tensor) -> torch.Tensor:
    """The torch composition of the length semantics: keys >= L masked out of the softmax, rows >= L zero.
    An all-padding sequence (L = 0) would make every softmax row -inf everywhere, hence NaN forward and
    backward: its scores are left unmasked instead (finite) and its rows are zeroed like any padded row."""
    B, S, D3 = qkv.shape
    dh = D3 // (3 * heads)
    q, k, v = qkv.view(B, S, 3, heads, dh).permute(2, 0, 3, 1, 4)
    L = lengths.clamp(0, S).view(B, 1, 1, 1)
    valid = torch.arange(S, device=qkv.device).view(1, 1, S) < L.view(B, 1, 1)  # [B, 1, S]
    s = (q @ k.transpose(-1, -2)) / math.sqrt(dh)
    s = s.masked_fill(~(valid.view(B, 1, 1, S) | (L == 0)), float("-inf"))
    a = F.dropout(torch.softmax(s, dim=-1), p) @ v  # [B, H, S, dh]
    a = a * valid.view(B, 1, S, 1).to(a.dtype)
    return a.transpose(1, 2).reshape(B, S, heads * dh)


def self_attention(qkv: torch.Tensor, heads: int, p: float = 0.0, lengths: torch.Tensor | None = None,
                   causal: bool = False, kv_heads: int | None = None, rope: float | None = None,
                   window: int | None = None) -> torch.Tensor:
    """softmax(Q K^T / sqrt(dh)) V with dropout ``p`` on the probabilities, per head (dh = 64 or 128 fused);
    ``qkv``: [B, S, 3*H*dh] -> [B, S, H*dh].  ``lengths`` (int32 [B], on qkv's device): the valid
    tokens of each padded sequence; ``causal``: query q attends to keys <= q; ``kv_heads``: grouped-query heads,
    ``qkv`` [B, S, (H + 2*kv_heads)*dh]; ``rope``: the base of rotary position embeddings on Q and K; ``window``:
    with ``causal``, only the keys q - window < k <= q (module docstring)."""
    B, S, D3 = qkv.shape
    if window is not None:
        return _window_attention(qkv, heads, p, lengths, causal, kv_heads, rope, window)
    if causal and lengths is not None:
        raise ValueError("self_attention: causal attention takes no lengths: right padding cannot reach a valid row")
    if rope is not None:
        return _rope_attention(qkv, heads, p, lengths, causal, kv_heads, rope)
    if kv_heads is not None:
        if kv_heads < 1 or heads % kv_heads:
            raise ValueError("self_attention: kv_heads must be at least 1 and divide heads, got heads %d, kv_heads %d"
                             % (heads, kv_heads))
        if lengths is not None:
            raise ValueError("self_attention: grouped-query attention (kv_heads) takes no lengths")
        if kv_heads != heads:  # (kv_heads == heads is the call without the keyword: the code below)
            return _gqa_attention(qkv, heads, kv_heads, p, causal)
    if lengths is not None:
        _check_lengths(qkv, lengths)
    if D3 == 3 * heads * 128 and eligible_d128(qkv, heads, lengths, causal):
        seed = int(torch.randint(0, 2**31 - 1, (1,)).item())  # CPU generator: no device sync
        dropout_seed.base(qkv.device)
        return _AttnD128Fn.apply(qkv, heads, float(p), seed, bool(causal))
    if eligible(qkv, heads, lengths, causal):
        seed = int(torch.randint(0, 2**31 - 1, (1,)).item())  # CPU generator: no device sync
        dropout_seed.base(qkv.device)  # registers the device seed word (graph replays advance it)
        if causal:
            return _AttnFn.apply(qkv, heads, float(p), seed, None, True)
        if lengths is None:
            return _AttnFn.apply(qkv, heads, float(p), seed)
        return _AttnFn.apply(qkv, heads, float(p), seed, lengths)
    if lengths is not None:
        return _lengths_fallback(qkv, heads, p, lengths)
    dh = D3 // (3 * heads)
    q, k, v = qkv.view(B, S, 3, heads, dh).permute(2, 0, 3, 1, 4)
    a = F.scaled_dot_product_attention(q, k, v, dropout_p=p, is_causal=causal)
    return a.transpose(1, 2).reshape(B, S, heads * dh)


def dropout_keep(seed: int, B: int, H: int, S: int, p: float, device=None, start: int = 0) -> torch.Tensor:
    """The kernels' keep mask [B, H, S(query), S(key)] (bool), computed with torch int64 ops; ``start``: of the queries
    and keys ``start .. start + S - 1`` of a longer sequence."""
    m32 = 0xFFFFFFFF
    bh = torch.arange(B * H, device=device, dtype=torch.int64).view(B * H, 1, 1)
    q = torch.arange(start, start + S, device=device, dtype=torch.int64).view(1, S, 1)
    k = torch.arange(start, start + S, device=device, dtype=torch.int64).view(1, 1, S)
    x = ((q << 16) | k) ^ seed
    x = (x * 0x9E3779B1) & m32
    x = x ^ (((bh * 0x85EBCA77) & m32) + (x >> 15)) & m32
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & m32
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & m32
    x = x ^ (x >> 16)
    thresh = 0 if p <= 0 else min(int(p * 4294967296.0), 0xFFFFFFFF)
    return (x >= thresh).view(B, H, S, S)
