"""Fused residual-add + RMSNorm on the HIP kernels of csrc/kernels/rmsnorm.hip: the norm of a pre-norm decoder block
(the LLaMA family).

``add_rms_norm(x, residual, weight, eps) -> (y, s)`` with ``s = x + residual`` (``x`` itself when ``residual`` is None)
and ``y = s * rsqrt(mean(s^2) + eps) * weight``.  Pre-norm uses both: ``y`` feeds the branch, ``s`` is the residual
stream that the next add continues from.  For bf16, contiguous GPU tensors with a supported row length (a multiple of
256 up to 8192) it is one HIP pass each way: ``s`` is rounded to bf16 once and normalised as stored, and the backward
adds the skip path's gradient of ``s`` inside the kernel, ahead of its one rounding, so summing the two gradients of
``s`` is no pass of its own.  Everything else (CPU, f32, other row lengths, ``_ENABLED = False``, the row lengths of
``_ROUTED_AWAY``) runs the torch composition of the same definition: f32 arithmetic, ``s`` rounded to the input dtype
before it is normalised.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn as nn

from .._lib import hip, hip_available

# False: every call runs the torch composition (tests and tools/bench_llama_block.py compare the paths in one process)
_ENABLED = True
# row lengths whose fused forward + backward did not beat the torch composition by more than the measured spread
# (profiles/llama_block.md): they keep the composition
_ROUTED_AWAY: frozenset = frozenset()


class _AddRMSNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, r, gamma, eps):
        from ..parallel.mixed import direct_target

        y, s, rstd = hip().rmsnorm_forward(x, r, gamma, eps)
        ctx.save_for_backward(s, gamma, rstd)
        ctx.has_r = r is not None
        ctx.direct = direct_target(gamma)
        return y, s  # without r, s is x itself

    @staticmethod
    def backward(ctx, dy, ds_skip):
        s, gamma, rstd = ctx.saved_tensors
        if dy is None:  # only the stream was used: its gradient passes through the add
            return ds_skip, (ds_skip if ctx.has_r else None), None, None
        if ds_skip is not None:
            ds_skip = ds_skip.contiguous()
        ds, dg = hip().rmsnorm_backward(dy.contiguous(), ds_skip, s, gamma, rstd)
        if ctx.direct is not None:
            # the gamma gradient to the flat space's sink (landed with its bucket, no AccumulateGrad add)
            from ..parallel.mixed import deliver

            deliver(ctx.direct, dg)
            dg = None
        # d(x + r)/dx = d(x + r)/dr = 1: both inputs receive the same ds
        return ds, (ds if ctx.has_r else None), dg, None


def eligible(x: torch.Tensor, r: Optional[torch.Tensor], w: torch.Tensor) -> bool:
    """Whether the fused kernels serve this call."""
    if not (_ENABLED and x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous() and x.numel() > 0
            and hip_available()):
        return False
    if r is not None and not (r.is_cuda and r.dtype == torch.bfloat16 and r.shape == x.shape and r.is_contiguous()):
        return False
    D = int(x.shape[-1])
    return (w.is_cuda and w.dtype == torch.float32 and w.shape == (D,) and D not in _ROUTED_AWAY
            and hip().rmsnorm_supported(D))


def add_rms_norm(x: torch.Tensor, residual: Optional[torch.Tensor], weight: torch.Tensor,
                 eps: float = 1e-6) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(y, s)``: ``s = x + residual`` in ``x``'s dtype and ``y = rms_norm(s) * weight`` in ``x``'s dtype."""
    if eligible(x, residual, weight):
        return _AddRMSNormFn.apply(x, residual, weight.contiguous(), float(eps))
    ct = torch.float64 if x.dtype == torch.float64 else torch.float32  # the arithmetic's dtype
    s = x if residual is None else (x.to(ct) + residual.to(ct)).to(x.dtype)
    sf = s.to(ct)
    y = sf * torch.rsqrt(sf.pow(2).mean(-1, keepdim=True) + eps) * weight
    return y.to(x.dtype), s


class AddRMSNorm(nn.Module):
    """``forward(x, residual=None) -> (y, s)`` of :func:`add_rms_norm` with an f32 ``weight`` of ones."""

    def __init__(self, D: int, eps: float = 1e-6):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(D))

    def forward(self, x, residual=None):
        if residual is not None and residual.dtype != x.dtype:
            residual = residual.to(x.dtype)
        return add_rms_norm(x, residual, self.weight, self.eps)
