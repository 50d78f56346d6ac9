"""Float64 numpy reference of the learner's optimizer step on one flat vector: the global-norm
clip scale, the Adam step and the centered-RMSprop step (csrc/kernels/optim.hip, csrc/adam_elem.h,
csrc/rms_pack.h).  The semantics are torch's -- ``torch.nn.utils.clip_grad_norm_``,
``torch.optim.Adam``, ``torch.optim.RMSprop(centered=True)`` -- which tests/test_optim_fast_cpu.py
checks; the GPU tests compare the kernels and the engine with it.

Every function takes and returns float64 arrays and changes none of its arguments.
"""
from __future__ import annotations

import numpy as np

CLIP_EPS = 1e-6     # clip_grad_norm_: max_norm / (norm + 1e-6)


def _f64(x) -> np.ndarray:
    return np.asarray(x, dtype=np.float64)


def grad_norm(g, gscale: float = 1.0) -> float:
    """Global L2 norm of ``gscale * g`` (gscale: 1 / world, the data-parallel average)."""
    g = _f64(g)
    return float(np.sqrt(np.sum(g * g))) * float(gscale)


def clip_scale(g, max_norm: float, gscale: float = 1.0) -> float:
    """The factor the update multiplies ``g`` by: ``gscale``, times ``max_norm / (norm + 1e-6)``
    when the norm of the scaled gradient exceeds ``max_norm`` (max_norm <= 0: no clipping)."""
    scale = float(gscale)
    if max_norm > 0:
        norm = grad_norm(g, gscale)
        if norm > max_norm:
            scale *= max_norm / (norm + CLIP_EPS)
    return scale


def adam_step(p, g, m, v, t: int, lr: float, b1: float = 0.9, b2: float = 0.999,
              eps: float = 1e-8, max_norm: float = 0.0, gscale: float = 1.0):
    """Step number ``t`` (1 for the first) of Adam, bias-corrected, eps outside the sqrt.
    Returns (p, m, v)."""
    p, m, v = _f64(p), _f64(m), _f64(v)
    gr = _f64(g) * clip_scale(g, max_norm, gscale)
    m = b1 * m + (1.0 - b1) * gr
    v = b2 * v + (1.0 - b2) * gr * gr
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    p = p - (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + eps)
    return p, m, v


def rmsprop_centered_step(p, g, sq, ga, lr: float, alpha: float = 0.95, eps: float = 1.5e-7,
                          max_norm: float = 0.0, gscale: float = 1.0):
    """One centered-RMSprop step (no momentum, no weight decay).  Returns (p, sq, ga)."""
    p, sq, ga = _f64(p), _f64(sq), _f64(ga)
    gr = _f64(g) * clip_scale(g, max_norm, gscale)
    sq = alpha * sq + (1.0 - alpha) * gr * gr
    ga = alpha * ga + (1.0 - alpha) * gr
    p = p - lr * gr / (np.sqrt(sq - ga * ga) + eps)
    return p, sq, ga
