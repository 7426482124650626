"""Gradient refinement of splat genomes: Adam over the device gradient.

``adam_step`` is the numpy statement of the update the device session
(``ga_device.DeviceRefine``, ggs_refine_* in include/ggs.h) performs; the device
is held to it bit for bit, given the same gradient.  ``refine`` runs a session.

The genome's columns live on different scales (positions in [0, 1], log-scales
of a few units, an angle, colours and alpha in [0, 255]), so the learning rate is
a vector, one entry per column.  ``DEFAULT_LR`` is a starting point — about one
percent of each column's range per step at full Adam step length — and has not
been tuned, just as DE's ``F`` and ``CR`` have not (§8b).
"""
from __future__ import annotations

import math
from typing import Dict, NamedTuple, Optional, Sequence

import numpy as np

from .ga import PI32, clamp_genome, scale_log_bounds, wrap_angle  # noqa: F401

_f32 = np.float32

# x, y, log a, log b, theta, r, g, b, alpha
DEFAULT_LR = (0.002, 0.002, 0.02, 0.02, 0.02, 2.0, 2.0, 2.0, 2.0)


class AdamParams(NamedTuple):
    lr: Sequence[float] = DEFAULT_LR
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-8
    log_lo: float = -np.inf          # clamp_genome's scale bounds (ga.scale_log_bounds)
    log_hi: float = np.inf


def bias_corrections(beta1: float, beta2: float, t: int):
    """float32(1 - beta^t), the power and the difference in float64 from the float32 beta."""
    b1, b2 = float(_f32(beta1)), float(_f32(beta2))
    return _f32(1.0 - math.pow(b1, float(t))), _f32(1.0 - math.pow(b2, float(t)))


def adam_step(x, g, m, v, t: int, params: AdamParams):
    """One Adam step on [..., 9] float32 arrays → (x, m, v), new arrays.  ``t`` is the
    step's number from 1.  Float32 throughout, every operation rounded once in the
    written order; then clamp_genome's rule per column, with an angle that is
    already inside [-pi, pi) keeping its bits (so a zero step changes nothing)."""
    if t < 1:
        raise ValueError("t counts steps from 1")
    x, g, m, v = (np.asarray(a, np.float32) for a in (x, g, m, v))
    lr = np.asarray(params.lr, np.float32).reshape(9)
    b1, b2, eps = _f32(params.beta1), _f32(params.beta2), _f32(params.eps)
    one = _f32(1.0)
    c1, c2 = bias_corrections(params.beta1, params.beta2, t)
    m = b1 * m + (one - b1) * g
    v = b2 * v + (one - b2) * (g * g)
    mh = m / c1
    den = np.sqrt(v / c2) + eps
    x = x - (lr * mh) / den
    x = x.astype(np.float32, copy=True)
    x[..., 0:2] = np.clip(x[..., 0:2], _f32(0.0), _f32(1.0))
    x[..., 2:4] = np.clip(x[..., 2:4], _f32(params.log_lo), _f32(params.log_hi))
    th = x[..., 4]
    inside = (th >= -PI32) & (th < PI32)
    x[..., 4] = np.where(inside, th, wrap_angle(th))
    x[..., 5:9] = np.clip(x[..., 5:9], _f32(0.0), _f32(255.0))
    return x, m.astype(np.float32), v.astype(np.float32)


def refine(genomes, target, H: int, W: int, steps: int, *, k_sigma: float = 3.0, weight_mask=None,
           boost_only: bool = False, boost_beta: float = 1.0, lr: Optional[Sequence[float]] = None,
           beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, min_scale_splats: float = 3.0,
           max_scale_splats: float = 0.1, device: int = 0, group: Optional[int] = None, loss=None,
           background=(1.0, 1.0, 1.0)) -> Dict[str, np.ndarray]:
    """``steps`` Adam steps on [B,N,9] (or [N,9]) genomes against ``target`` on the
    device → ``DeviceRefine.read``'s dict: the final state and its fitness, and per
    candidate the best state seen (``best`` / ``best_fits``), which is what a polish
    keeps.  ``lr=None``: ``DEFAULT_LR``.  A 4-D ``target`` [K,H,W,3] (``weight_mask``
    [K,H,W]) refines candidate b against image ``b // group`` in one session.
    ``loss`` (``ggs.LossParams``; default None: the fitness) descends the image loss
    L1 / MSE / SSIM of the render against ``background`` instead."""
    from .ga_device import DeviceRefine
    tgt = np.ascontiguousarray(target, np.float32)
    if tgt.shape[-3:] != (int(H), int(W), 3) or tgt.ndim not in (3, 4):
        raise ValueError(f"target must be [H,W,3] or [K,H,W,3] with (H, W) = {(H, W)}, got {tuple(tgt.shape)}")
    s = DeviceRefine(tgt, weight_mask, genomes, lr=DEFAULT_LR if lr is None else lr, beta1=beta1, beta2=beta2,
                     eps=eps, min_scale_splats=min_scale_splats, max_scale_splats=max_scale_splats,
                     k_sigma=k_sigma, boost_only=boost_only, boost_beta=boost_beta, device=device, group=group, loss=loss,
                     background=background)
    try:
        s.run(int(steps))
        return s.read()
    finally:
        s.close()
