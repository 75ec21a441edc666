"""Layer-wise trust-ratio optimizers: LARS and LAMB.

The large-batch companions of everything here that grows the global batch at run time (elastic
resize, the gradient-noise-scale monitor, ``AdaptiveSGDOptimizer``, the batch-size policies): each
tensor's step is scaled by a ratio of its weight norm to its update norm.  The reference has neither;
the definitions below are the specification.  Per tensor *k*, with ``g = grad * grad_scale``:

LARS
    ``q = trust_coefficient * |w| / (|g| + wd_k * |w| + eps)`` where trust is on and both norms are
    non-zero, else 1; ``d = q * (g + wd_k * w)``; ``m <- momentum * m + d`` (``m`` starts at zero);
    ``w <- w - lr * (d + momentum * m if nesterov else m)``.

LAMB
    ``g`` is first multiplied by ``min(1, max_grad_norm / |g_all|)`` when ``max_grad_norm`` is set
    (``|g_all|``: the norm of the whole scaled gradient); ``m <- b1 * m + (1 - b1) * g``;
    ``v <- b2 * v + (1 - b2) * g^2``; ``u = mhat / (sqrt(vhat) + eps) + wd_k * w`` with the moments
    bias-corrected by the step count when ``bias_correction``; ``r = |w| / |u|`` where trust is on
    and both norms are non-zero, else 1; ``w <- w - lr * r * u``.

:class:`LARS` / :class:`LAMB` are plain ``torch.optim.Optimizer`` s in torch ops, one tensor at a
time: the semantic reference, and what runs on CPU or with ``fused=False``.  Param groups may
override ``weight_decay`` and a boolean ``trust``; the usual "no decay, no adaptation for biases and
norm parameters" group is ``dict(params=..., weight_decay=0.0, trust=False)``.

:class:`FusedLARS` / :class:`FusedLAMB` run the same step over a :class:`FlatParamSpace` in three
launches (``csrc/kernels/layerwise.hip``): per-chunk partial norms, per-slot coefficients, apply.
No host sync, no float atomics, fixed launch shapes, so a hipGraph replays it; the per-slot norms
and ratios of the last step are device tensors (:meth:`trust_ratios`).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .._lib import hip
from ..parallel.flat import FlatParamSpace


# -- the update in torch ops (the plain optimizers per tensor, the fused classes' CPU path per slot) ---------

def _ratio(trust: bool, num: torch.Tensor, den: torch.Tensor, wn: torch.Tensor, xn: torch.Tensor) -> torch.Tensor:
    """num / den where trust is on and both norms are non-zero, else 1 (a 0-dim tensor: no host sync)."""
    one = torch.ones_like(wn)
    if not trust:
        return one
    return torch.where((wn > 0) & (xn > 0), num / den, one)


def _lars_update(w, g, m, lr, mu, wd, tc, eps, nesterov, trust):
    """One LARS step on (w, m) in place; m is None when mu == 0.  Returns (|w|, |g|, q)."""
    wn, gn = w.norm(), g.norm()
    q = _ratio(trust, tc * wn, gn + wd * wn + eps, wn, gn)
    d = g.add(w, alpha=wd) if wd else g
    d = d * q
    if m is not None:
        m.mul_(mu).add_(d)
        d = d.add(m, alpha=mu) if nesterov else m
    w.add_(d, alpha=-lr)
    return wn, gn, q


def _lamb_update(w, g, m, v, t, lr, b1, b2, eps, wd, bias_correction, trust):
    """One LAMB step on (w, m, v) in place; t is the step count.  Returns (|w|, |u|, r)."""
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    bc1 = 1 - b1 ** t if bias_correction else 1.0
    bc2 = 1 - b2 ** t if bias_correction else 1.0
    u = (m / bc1) / ((v / bc2).sqrt_().add_(eps))
    if wd:
        u.add_(w, alpha=wd)
    wn, un = w.norm(), u.norm()
    r = _ratio(trust, wn, un, wn, un)
    w.sub_(u * (lr * r))
    return wn, un, r


def _clip_factor(sumsq: torch.Tensor, max_grad_norm: float) -> torch.Tensor:
    return (max_grad_norm / sumsq.sqrt()).clamp(max=1.0)  # x / 0 = inf: no clipping


class LARS(torch.optim.Optimizer):
    """Layer-wise adaptive rate scaling (You, Gitman, Ginsburg 2017), per tensor in torch ops."""

    def __init__(self, params, lr: float, momentum: float = 0.9, weight_decay: float = 0.0,
                 trust_coefficient: float = 0.001, eps: float = 1e-8, nesterov: bool = False):
        if lr < 0 or momentum < 0 or weight_decay < 0 or trust_coefficient <= 0:
            raise ValueError("LARS: lr, momentum, weight_decay must be >= 0 and trust_coefficient > 0")
        defaults = dict(lr=lr, momentum=momentum, weight_decay=weight_decay, trust_coefficient=trust_coefficient,
                        eps=eps, nesterov=nesterov, trust=True)
        super().__init__(params, defaults)
        self.grad_scale = 1.0

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gr in self.param_groups:
            for p in gr["params"]:
                if p.grad is None:
                    continue
                g = p.grad * self.grad_scale if self.grad_scale != 1.0 else p.grad
                m = None
                if gr["momentum"]:
                    st = self.state[p]
                    if "momentum_buffer" not in st:
                        st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    m = st["momentum_buffer"]
                _lars_update(p, g, m, gr["lr"], gr["momentum"], gr["weight_decay"], gr["trust_coefficient"],
                             gr["eps"], gr["nesterov"], gr["trust"])
        return loss


class LAMB(torch.optim.Optimizer):
    """Layer-wise adaptive moments (You et al. 2020), per tensor in torch ops."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-6, weight_decay: float = 0.0,
                 bias_correction: bool = True, max_grad_norm: Optional[float] = None):
        if lr < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1) or weight_decay < 0:
            raise ValueError("LAMB: lr, weight_decay must be >= 0 and betas in [0, 1)")
        if max_grad_norm is not None and max_grad_norm <= 0:
            raise ValueError("LAMB: max_grad_norm must be positive (or None)")
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, bias_correction=bias_correction,
                        max_grad_norm=max_grad_norm, trust=True)
        super().__init__(params, defaults)
        self.grad_scale = 1.0

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        clip = None
        mgn = self.param_groups[0]["max_grad_norm"]
        if mgn is not None:
            grads = [p.grad for gr in self.param_groups for p in gr["params"] if p.grad is not None]
            if grads:
                sumsq = torch.stack([g.double().square().sum() for g in grads]).sum() * self.grad_scale ** 2
                clip = _clip_factor(sumsq, mgn).to(grads[0].dtype)
        for gr in self.param_groups:
            b1, b2 = gr["betas"]
            for p in gr["params"]:
                if p.grad is None:
                    continue
                g = p.grad * self.grad_scale if self.grad_scale != 1.0 else p.grad
                if clip is not None:
                    g = g * clip
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                _lamb_update(p, g, st["exp_avg"], st["exp_avg_sq"], st["step"], gr["lr"], b1, b2, gr["eps"],
                             gr["weight_decay"], gr["bias_correction"], gr["trust"])
        return loss


# -- the flat space: slots, chunks, per-slot tables ---------------------------------------------------------

def slot_offsets(space: FlatParamSpace) -> List[int]:
    """The nseg + 1 slot starts of ``space``: slot k spans [off[k], off[k+1]) with its alignment padding."""
    return [o for o, _ in space.offsets] + [space.numel]


def chunk_map(offsets: Sequence[int], chunk: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Cut every slot into chunks of at most ``chunk`` elements that never cross a slot boundary.

    Returns ``chunks`` (int64 [nchunks, 3]: first element, slot, length) in slot order and
    ``slot_chunk0`` (int64 [nseg + 1]: first chunk of each slot), both on the CPU."""
    rows, first = [], [0]
    for k in range(len(offsets) - 1):
        lo, hi = int(offsets[k]), int(offsets[k + 1])
        if hi <= lo:
            raise ValueError("chunk_map: slot offsets must be ascending")
        for s in range(lo, hi, chunk):
            rows.append((s, k, min(chunk, hi - s)))
        first.append(len(rows))
    return (torch.tensor(rows, dtype=torch.int64).reshape(-1, 3), torch.tensor(first, dtype=torch.int64))


class _LayerwiseBase(torch.optim.Optimizer):
    """What FusedLARS and FusedLAMB share: the slot tables, the norm outputs, the flat-view plumbing.

    ``weight_decay`` (with ``overrides``) and ``trust`` become per-slot device tables here, at construction;
    the learning rate and the other scalars are read from ``param_groups[0]`` on every step."""

    def __init__(self, space: FlatParamSpace, defaults: dict, overrides: Optional[Dict], grad_scale: float):
        super().__init__(space.params, defaults)
        self.space = space
        self.grad_scale = grad_scale
        dev = space.device
        nseg = len(space.params)
        wd = [float(defaults["weight_decay"])] * nseg
        trust = [1.0] * nseg
        for p, o in (overrides or {}).items():
            k = space.index(p)
            unknown = set(o) - {"weight_decay", "trust"}
            if unknown:
                raise ValueError("overrides: unknown keys %s" % sorted(unknown))
            wd[k] = float(o.get("weight_decay", wd[k]))
            trust[k] = 1.0 if o.get("trust", True) else 0.0
        self.wd_tab = torch.tensor(wd, dtype=torch.float32, device=dev)
        self.trust_tab = torch.tensor(trust, dtype=torch.float32, device=dev)
        self.w_norm = torch.zeros(nseg, dtype=torch.float32, device=dev)
        self.x_norm = torch.zeros(nseg, dtype=torch.float32, device=dev)
        self.ratio = torch.ones(nseg, dtype=torch.float32, device=dev)
        self._lr_t = torch.full((1,), float(defaults["lr"]), dtype=torch.float32, device=dev)
        self._offsets = torch.tensor(slot_offsets(space), dtype=torch.int64)  # host: the binding checks it
        self._gpu = dev.type == "cuda"
        if self._gpu:
            chunks, first = chunk_map(self._offsets.tolist(), hip().layerwise_chunk)
            self._chunks = chunks.to(dev)
            self._slot_chunk0 = first.to(dev)
            self._partials = torch.zeros(2 * chunks.shape[0], dtype=torch.float32, device=dev)
        else:  # per-slot host copies for the torch-op path
            self._wd, self._trust = wd, [t != 0.0 for t in trust]

    def zero_grad(self, set_to_none: bool = False):  # keep the flat grad views
        self.space.zero_grad()

    def trust_ratios(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(|w|, |g| for LARS or |u| for LAMB, ratio applied) per slot, as of the last step: three
        device tensors in the order of ``space.params``; reading them makes no sync here."""
        return self.w_norm, self.x_norm, self.ratio

    def _tables(self):
        return (self._offsets, self._chunks, self._slot_chunk0, self._partials, self.wd_tab, self.trust_tab,
                self.w_norm, self.x_norm, self.ratio)

    def _eager_shadow(self):
        # the bf16 compute shadow is written by the apply kernel on eager steps (as FusedAdam does)
        sp = self.space
        if sp.flat_shadow is not None and not torch.cuda.is_current_stream_capturing():
            return sp.flat_shadow
        return None

    def _slots(self):
        sp = self.space
        off = self._offsets.tolist()
        return [(k, slice(off[k], off[k + 1])) for k in range(len(sp.params))]

    def _record(self, k, wn, xn, r):
        self.w_norm[k], self.x_norm[k], self.ratio[k] = wn, xn, r

    def _flat_state(self) -> dict:
        raise NotImplementedError

    def state_dict(self):
        sd = super().state_dict()
        sd["kungfu_flat"] = self._flat_state()
        return sd

    def load_state_dict(self, sd):
        flat = sd.pop("kungfu_flat", None)
        super().load_state_dict(sd)
        if flat is not None:
            mine = self._flat_state()
            for k, v in flat.items():
                if v is not None and mine.get(k) is not None:
                    mine[k].copy_(v)


class FusedLARS(_LayerwiseBase):
    """LARS over a flat space: three launches per step for the whole model (28 B of HBM traffic per
    parameter against FusedSGD's 20)."""

    def __init__(self, space: FlatParamSpace, lr: float = 0.01, momentum: float = 0.9, weight_decay: float = 0.0,
                 trust_coefficient: float = 0.001, eps: float = 1e-8, nesterov: bool = False,
                 overrides: Optional[Dict] = None, grad_scale: float = 1.0):
        defaults = dict(lr=lr, momentum=momentum, weight_decay=weight_decay, trust_coefficient=trust_coefficient,
                        eps=eps, nesterov=nesterov)
        super().__init__(space, defaults, overrides, grad_scale)
        self.momentum_buffer = torch.zeros_like(space.flat_param) if momentum else None

    def _flat_state(self):
        return {"momentum_buffer": self.momentum_buffer}

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        g = self.param_groups[0]
        lr, mu, tc, eps, nes = g["lr"], g["momentum"], g["trust_coefficient"], g["eps"], g["nesterov"]
        sp = self.space
        if self._gpu:
            if not torch.cuda.is_current_stream_capturing():  # replays get it from GraphedStep.pre_replay
                self._lr_t.fill_(lr)
            sh = self._eager_shadow()
            hip().lars_step(sp.flat_param, sp.flat_grad, self.momentum_buffer, sh, *self._tables(), lr, self._lr_t,
                            mu, tc, eps, self.grad_scale, nes)
            if sh is not None:
                sp.mark_shadow_fresh()
        else:
            for k, s in self._slots():
                gr = sp.flat_grad[s] * self.grad_scale
                m = self.momentum_buffer[s] if self.momentum_buffer is not None else None
                self._record(k, *_lars_update(sp.flat_param[s], gr, m, lr, mu, self._wd[k], tc, eps, nes,
                                              self._trust[k]))
        return loss


class FusedLAMB(_LayerwiseBase):
    """LAMB over a flat space: three launches per step (40 B of HBM traffic per parameter against
    FusedAdam's 28), one more pass over the gradient when ``max_grad_norm`` is set."""

    def __init__(self, space: FlatParamSpace, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-6,
                 weight_decay: float = 0.0, bias_correction: bool = True, max_grad_norm: Optional[float] = None,
                 overrides: Optional[Dict] = None, grad_scale: float = 1.0):
        if max_grad_norm is not None and max_grad_norm <= 0:
            raise ValueError("FusedLAMB: max_grad_norm must be positive (or None)")
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, bias_correction=bias_correction,
                        max_grad_norm=max_grad_norm)
        super().__init__(space, defaults, overrides, grad_scale)
        self.exp_avg = torch.zeros_like(space.flat_param)
        self.exp_avg_sq = torch.zeros_like(space.flat_param)
        self._step_t = torch.zeros(1, dtype=torch.float32, device=space.device)
        # scratch of the whole-gradient sum of squares (sumsq2's partials + its 2 results)
        self._gnorm_ws = None
        if self._gpu and max_grad_norm is not None:
            self._gnorm_ws = torch.zeros(2 * hip().layerwise_grid_cap + 2, dtype=torch.float32, device=space.device)

    def _flat_state(self):
        return {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq, "step": self._step_t}

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        g = self.param_groups[0]
        lr, (b1, b2), eps, bc, mgn = g["lr"], g["betas"], g["eps"], g["bias_correction"], g["max_grad_norm"]
        sp = self.space
        self._step_t.add_(1.0)
        if self._gpu:
            if mgn is not None and self._gnorm_ws is None:
                raise RuntimeError("FusedLAMB: max_grad_norm was None at construction and cannot be set later")
            if not torch.cuda.is_current_stream_capturing():
                self._lr_t.fill_(lr)
            sh = self._eager_shadow()
            hip().lamb_step(sp.flat_param, sp.flat_grad, self.exp_avg, self.exp_avg_sq, sh, *self._tables(), lr,
                            self._lr_t, b1, b2, eps, self.grad_scale, self._step_t, bc,
                            0.0 if mgn is None else mgn, self._gnorm_ws)
            if sh is not None:
                sp.mark_shadow_fresh()
        else:
            t = int(round(float(self._step_t.item())))
            scale = self.grad_scale
            if mgn is not None:
                sumsq = sp.flat_grad.double().square().sum() * self.grad_scale ** 2
                scale = self.grad_scale * _clip_factor(sumsq, mgn).to(sp.flat_grad.dtype)
            for k, s in self._slots():
                gr = sp.flat_grad[s] * scale
                self._record(k, *_lamb_update(sp.flat_param[s], gr, self.exp_avg[s], self.exp_avg_sq[s], t, lr, b1,
                                              b2, eps, self._wd[k], bc, self._trust[k]))
        return loss


# -- routing from the plain optimizers (optimizers/core.py make_fused) --------------------------------------

_PER_GROUP = ("params", "weight_decay", "trust")


def fused_from(optimizer: torch.optim.Optimizer, space: FlatParamSpace):
    """The fused equivalent of a plain LARS / LAMB, or None when its param groups differ in more than
    ``weight_decay`` / ``trust`` (per-slot tables carry those two; everything else is one scalar)."""
    groups = optimizer.param_groups
    base = groups[0]
    for gr in groups[1:]:
        if set(gr) != set(base) or any(gr[k] != base[k] for k in base if k not in _PER_GROUP):
            return None
    overrides = None
    if len(groups) > 1 or not base.get("trust", True):
        overrides = {p: dict(weight_decay=gr["weight_decay"], trust=gr.get("trust", True))
                     for gr in groups for p in gr["params"] if p.requires_grad}
    gs = getattr(optimizer, "grad_scale", 1.0)
    if type(optimizer) is LARS:
        return FusedLARS(space, lr=base["lr"], momentum=base["momentum"], weight_decay=base["weight_decay"],
                         trust_coefficient=base["trust_coefficient"], eps=base["eps"], nesterov=base["nesterov"],
                         overrides=overrides, grad_scale=gs)
    if type(optimizer) is LAMB:
        return FusedLAMB(space, lr=base["lr"], betas=base["betas"], eps=base["eps"],
                         weight_decay=base["weight_decay"], bias_correction=base["bias_correction"],
                         max_grad_norm=base["max_grad_norm"], overrides=overrides, grad_scale=gs)
    return None
