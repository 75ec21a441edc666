"""A LLaMA-family decoder: pre-norm blocks of RMSNorm, grouped-query causal attention with rotary position embeddings
at head dim 128, and a SwiGLU FFN; no biases, no dropout, no position table, tied output embedding.  The default is a
small model of the family's shape (d = 1024, 12 layers, 8 heads of 128 over 2 K/V heads, FFN 2816, vocab 32000).
``window=W`` (a multiple of 64; Mistral: 4096) makes every layer's attention local: a token sees the last ``W`` tokens,
itself included (ops/attention.py: sliding-window attention, sequences up to 8192 tokens on the band kernels).

Every pass that is not a GEMM runs on this project's HIP kernels under bf16 autocast on the GPU: the attention of
``gpt_rope`` (csrc/kernels/attention_rope.hip, attention_d128.hip), both norms with the residual adds inside them
(ops/rmsnorm.py, csrc/kernels/rmsnorm.hip) and the FFN activation (ops/swiglu.py, csrc/kernels/swiglu.hip).  A layer
takes the residual stream ``x`` and the previous branch's output ``delta`` that has not been added yet, and returns the
pair again: every residual add of the model happens inside a norm kernel, the final norm's included.
``lm_loss`` and ``synthetic_lm_batch`` of models/gpt.py work on it unchanged."""
import torch
import torch.nn as nn

from ..ops.attention import self_attention
from ..ops.embedding import embedding
from ..ops.rmsnorm import AddRMSNorm
from ..ops.swiglu import swiglu
from ..ops.vocab import vocab_projection


class LlamaLayer(nn.Module):
    def __init__(self, d=1024, heads=8, kv_heads=2, ffn=2816, rope=10000.0, eps=1e-6, window=None):
        super().__init__()
        if d % heads or heads % kv_heads:
            raise ValueError("LlamaLayer: heads must divide d and kv_heads must divide heads, got d %d, heads %d, "
                             "kv_heads %d" % (d, heads, kv_heads))
        self.heads, self.kv_heads, self.rope, self.window = heads, kv_heads, rope, window
        self.norm1 = AddRMSNorm(d, eps)
        # one projection of the query, key and value heads (ops/attention.py's grouped-query layout)
        self.qkv = nn.Linear(d, (heads + 2 * kv_heads) * (d // heads), bias=False)
        self.out = nn.Linear(d, d, bias=False)
        self.norm2 = AddRMSNorm(d, eps)
        # one projection of gate and up: gate in the first ffn columns, up in the last (ops/swiglu.py)
        self.gate_up = nn.Linear(d, 2 * ffn, bias=False)
        self.down = nn.Linear(ffn, d, bias=False)

    def forward(self, x, delta=None):
        """``(stream, branch output not yet added)`` from the same pair (``delta`` None: nothing to add)."""
        y, s = self.norm1(x, delta)
        a = self.out(self_attention(self.qkv(y), self.heads, 0.0, causal=True, kv_heads=self.kv_heads, rope=self.rope,
                                    window=self.window))
        y2, s2 = self.norm2(s, a)
        m = self.down(swiglu(self.gate_up(y2)))
        return s2, m


class LlamaLM(nn.Module):
    def __init__(self, vocab=32000, d=1024, layers=12, heads=8, kv_heads=2, ffn=2816, rope=10000.0, eps=1e-6,
                 window=None):
        super().__init__()
        self.tok = nn.Embedding(vocab, d)
        self.layers = nn.ModuleList([LlamaLayer(d, heads, kv_heads, ffn, rope, eps, window) for _ in range(layers)])
        self.norm = AddRMSNorm(d, eps)
        self.apply(self._init)

    @staticmethod
    def _init(m):
        if isinstance(m, (nn.Linear, nn.Embedding)):
            nn.init.normal_(m.weight, std=0.02)

    def forward(self, ids):
        """Next-token logits [B, S, vocab] of token ids [B, S]."""
        x = embedding(ids, self.tok.weight)
        if torch.is_autocast_enabled(x.device.type) and x.is_cuda:
            x = x.to(torch.get_autocast_dtype(x.device.type))  # bf16 residual stream from here on, as in GPTLM
        delta = None
        for layer in self.layers:
            x, delta = layer(x, delta)
        y, _ = self.norm(x, delta)  # the last branch is added inside the final norm
        # tied output embedding, no bias; gemm.hip's ragged-N GEMM with padded logits rows (ops/vocab.py)
        return vocab_projection(y, self.tok.weight)


def llama(**kw):
    kw.pop("fused_bn", None)
    return LlamaLM(**kw)
