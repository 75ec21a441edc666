"""SwiGLU on the HIP kernels of csrc/kernels/swiglu.hip: ``swiglu(gu) = silu(gate) * up`` for ``gu [..., 2F]``, the
output of one ``Linear(d, 2F)`` whose first ``F`` columns are the gate and whose last ``F`` are the up projection.

For bf16, contiguous GPU tensors with ``F % 8 == 0`` it is one HIP pass each way over the ``[tokens, ffn]``
activations, the largest tensors of a decoder layer: the forward writes ``h`` once, the backward recomputes the sigmoid
from ``gu`` (``h`` is not saved) and writes both halves of ``dgu`` once, in ``gu``'s layout, with no concatenation.
Everything else (CPU, f32, other ``F``, ``_ENABLED = False``, the ``F`` of ``_ROUTED_AWAY``) runs the torch composition
``F.silu(gate.float()) * up.float()`` rounded once to the input dtype.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .._lib import hip, hip_available

# False: every call runs the torch composition (tests and tools/bench_llama_block.py compare the paths in one process)
_ENABLED = True
# F whose fused forward + backward did not beat the torch composition by more than the measured spread
# (profiles/llama_block.md): they keep the composition
_ROUTED_AWAY: frozenset = frozenset()


class _SwiGLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gu):
        ctx.save_for_backward(gu)
        return hip().swiglu_forward(gu)

    @staticmethod
    def backward(ctx, dh):
        (gu,) = ctx.saved_tensors
        return hip().swiglu_backward(dh.contiguous(), gu)


def eligible(gu: torch.Tensor) -> bool:
    """Whether the fused kernels serve this call."""
    return (_ENABLED and gu.is_cuda and gu.dtype == torch.bfloat16 and gu.dim() >= 1 and gu.is_contiguous()
            and gu.numel() > 0 and gu.shape[-1] % 16 == 0 and gu.shape[-1] // 2 not in _ROUTED_AWAY
            and hip_available())


def swiglu(gu: torch.Tensor) -> torch.Tensor:
    """``silu(gu[..., :F]) * gu[..., F:]`` with ``F = gu.shape[-1] // 2``, in ``gu``'s dtype."""
    if gu.shape[-1] % 2:
        raise ValueError("swiglu: the last dim must be even (gate and up halves), got %d" % gu.shape[-1])
    if eligible(gu):
        return _SwiGLUFn.apply(gu)
    g, u = gu.chunk(2, dim=-1)
    if gu.dtype == torch.float64:
        return F.silu(g) * u
    return (F.silu(g.float()) * u.float()).to(gu.dtype)
