"""GPT (the 2018 decoder-only Transformer language model): 12 post-LN layers, hidden 768, 12 heads of 64,
FFN 3072, GELU, learned positions, a context of 512 tokens, vocab 40478, tied output embedding, ~116 M
parameters.  Architecturally BERT's encoder layer with a causal mask: the layers are ``BertLayer``s called
with ``causal=True``, whose attention runs the triangular fused HIP kernels of ops/attention.py (S a multiple
of 64 up to 1024; anything else ``F.scaled_dot_product_attention(is_causal=True)``).  The head dim is ``d / heads``:
64 and 128 have fused kernels.  ``gpt_d128`` is the same model with GPT-3 / LLaMA-style heads of 128: d = 1024, 8 heads,
FFN 4096, whose attention runs csrc/kernels/attention_d128.hip; ``gpt_gqa`` is ``gpt_d128`` with LLaMA-2-style
grouped-query attention (``kv_heads=2``: the same kernels with groups of 4 heads); ``gpt_rope`` is ``gpt_gqa`` with rotary
position embeddings of base 10000 on Q and K instead of the learned position table (``rope=10000.0``: the LLaMA-2
attention block; csrc/kernels/attention_rope.hip and the grouped-query backward's epilogues)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops.embedding import embedding
from ..ops.vocab import vocab_projection
from ..ops.xent import cross_entropy
from .bert import BertLayer


class GPTLM(nn.Module):
    def __init__(self, vocab=40478, d=768, layers=12, heads=12, ffn=3072, max_pos=512, dropout=0.1, kv_heads=None,
                 rope=None):
        super().__init__()
        self.tok = nn.Embedding(vocab, d)
        if rope is None:
            self.pos = nn.Embedding(max_pos, d)
            self.layers = nn.ModuleList([BertLayer(d, heads, ffn, dropout, kv_heads) for _ in range(layers)])
        else:  # rotary embeddings in every layer's attention: no position table (max_pos is unused)
            self.pos = None
            self.layers = nn.ModuleList([BertLayer(d, heads, ffn, dropout, kv_heads, rope) for _ in range(layers)])
        self.dropout = dropout
        self.apply(self._init)

    @staticmethod
    def _init(m):
        if isinstance(m, (nn.Linear, nn.Embedding)):
            nn.init.normal_(m.weight, std=0.02)
        if isinstance(m, nn.Linear) and m.bias is not None:
            nn.init.zeros_(m.bias)

    def forward(self, ids):
        """Next-token logits [B, S, vocab] of token ids [B, S] (S <= max_pos)."""
        B, S = ids.shape
        # scatter-add embedding gradients (ops/embedding.py): fixed-shape, graph-replayable
        x = embedding(ids, self.tok.weight)
        if self.pos is not None:  # (None: rotary embeddings inside the layers)
            x = x + embedding(torch.arange(S, device=ids.device), self.pos.weight)[None]
        if torch.is_autocast_enabled(x.device.type) and x.is_cuda:
            x = x.to(torch.get_autocast_dtype(x.device.type))  # bf16 residual stream from here on, as in BERT
        x = F.dropout(x, self.dropout, self.training)
        for layer in self.layers:
            x = layer(x, causal=True)
        # tied output embedding, no bias; gemm.hip's ragged-N GEMM with padded logits rows (ops/vocab.py)
        return vocab_projection(x, self.tok.weight)


def gpt_base(**kw):
    kw.pop("fused_bn", None)
    return GPTLM(**kw)


def gpt_d128(**kw):
    """GPTLM with 8 heads of 128 (d = 1024, FFN 4096); the remaining defaults are GPTLM's."""
    kw.pop("fused_bn", None)
    return GPTLM(**{"d": 1024, "heads": 8, "ffn": 4096, **kw})


def gpt_gqa(**kw):
    """``gpt_d128`` with grouped-query attention: its 8 query heads of 128 share 2 K/V heads (groups of 4)."""
    return gpt_d128(**{"kv_heads": 2, **kw})


def gpt_rope(**kw):
    """``gpt_gqa`` with rotary position embeddings (base 10000) in place of the learned position table."""
    return gpt_gqa(**{"rope": 10000.0, **kw})


def synthetic_lm_batch(batch: int, seq_len: int = 512, vocab: int = 40478, device=None, generator=None):
    """Random token ids [batch, seq_len] of a language-model batch."""
    return torch.randint(0, vocab, (batch, seq_len), device=device, generator=generator)


def lm_loss(model, ids):
    """Mean next-token cross-entropy: positions 0 .. S-2 predict ids[:, 1:] (ops/xent.py on bf16 logits)."""
    logits = model(ids)
    return cross_entropy(logits[:, :-1], ids[:, 1:])
