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


class DensityParams(NamedTuple):
    """Density control of a refine session (ggs_refine_density): every
    ``every`` steps from ``start`` to ``stop`` (0: no end), each candidate's dead splats
    (alpha below ``alpha_dead``) are relocated onto its live splats whose accumulated
    positional gradient per step exceeds ``grad_min``, at most ``max_moves`` of them: as
    clones when the larger log-scale is at most ``split_log``, else as halves of a split
    ``split_offset`` sigmas apart with both scales divided by ``shrink``.  N never changes.
    The defaults are starting values (the shrink is 3DGS's 1.6) and have not been tuned,
    just as ``DEFAULT_LR`` has not.  ``grad_min = 0`` makes every live splat with a
    gradient a source, so the ranking alone chooses: 3DGS's 0.0002 is a threshold for its
    screen-space gradients and lies above anything the normalised fitness produces here
    (docs/EXPERIMENTS.md §31: no splat ever qualified).  ``every = 0`` is off, which is
    also what a session without them does."""
    every: int = 100
    start: int = 100
    stop: int = 0
    max_moves: int = 64
    alpha_dead: float = 2.0
    grad_min: float = 0.0
    split_log: float = 2.0
    shrink: float = 1.6
    split_offset: float = 0.5


def density_params_c(params) -> "_lib.RefineDensity":
    """ggs_refine_density of a ``DensityParams`` (or its nine values in order), with
    ``log_shrink = float32(log(shrink))``.  The rules of ggs_refine_set_density are
    checked here as well, so a bad value is refused whatever it is handed to."""
    from . import _lib
    p = params if isinstance(params, DensityParams) else DensityParams(*params)
    ints = {k: getattr(p, k) for k in ("every", "start", "stop", "max_moves")}
    for k, val in ints.items():
        if int(val) != val or val < 0 or val >= 2 ** 31:
            raise _lib.GGSInputError(f"density: {k}={val!r} must be an integer in [0, 2^31)")
    if p.every > 0 and p.max_moves == 0:
        raise _lib.GGSInputError("density: max_moves must be >= 1 when every > 0")
    floats = {k: float(getattr(p, k)) for k in ("alpha_dead", "grad_min", "split_log", "shrink", "split_offset")}
    for k, val in floats.items():
        if not math.isfinite(val) or abs(val) > float(np.finfo(np.float32).max):
            raise _lib.GGSInputError(f"density: {k}={val!r} must be finite")
    if not 0.0 <= floats["alpha_dead"] <= 255.0:
        raise _lib.GGSInputError(f"density: alpha_dead={p.alpha_dead!r} must be in [0, 255]")
    if floats["grad_min"] < 0.0:
        raise _lib.GGSInputError(f"density: grad_min={p.grad_min!r} must be >= 0")
    if floats["shrink"] < 1.0:
        raise _lib.GGSInputError(f"density: shrink={p.shrink!r} must be >= 1")
    return _lib.RefineDensity(int(p.every), int(p.start), int(p.stop), int(p.max_moves), floats["alpha_dead"],
                              floats["grad_min"], floats["split_log"], float(_f32(math.log(floats["shrink"]))),
                              floats["split_offset"])


def density_moves(params, N: int) -> int:
    """The effective ``max_moves`` of N splats: min(max_moves, N // 2); 0 when off."""
    return min(int(params.max_moves), int(N) // 2) if int(params.every) > 0 else 0


def density_accumulate(acc, grad, H: int, W: int) -> np.ndarray:
    """``acc`` [..., N] plus the per-pixel norm of ``grad`` [..., N, 9]'s position columns →
    a new float32 array: what the device adds on every step while density control is on."""
    acc, g = np.asarray(acc, np.float32), np.asarray(grad, np.float32)
    px = g[..., 0] / _f32(max(int(W) - 1, 1))
    py = g[..., 1] / _f32(max(int(H) - 1, 1))
    return (acc + np.sqrt(px * px + py * py)).astype(np.float32)


def _library_detmath(fn: int, x: np.ndarray) -> np.ndarray:
    import ctypes as C
    from . import _lib
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    fp = C.POINTER(C.c_float)
    _lib.check(_lib.lib.ggs_detmath_eval(fn, x.ctypes.data_as(fp), None, x.size, out.ctypes.data_as(fp)),
               "ggs_detmath_eval")
    return out


def relocate(x, m, v, acc, n_acc: int, H: int, W: int, params, log_lo: float, log_hi: float, *, detmath=None):
    """One density-control event (include/ggs.h, ggs_refine_density) on [B, N, 9] (or
    [N, 9]) float32 ``x``, ``m``, ``v`` and ``acc`` [B, N] ([N]) → new ``(x, m, v, pairs,
    is_split)``: ``pairs`` int32 [B, M, 2] ([M, 2]) holds the (dead, source) rows of the
    pairs moved and (-1, -1) after them, ``is_split`` int32 [B, M] ([M]) which of them
    were splits, M = ``density_moves(params, N)``.  Zeroing ``acc`` and ``n_acc``
    afterwards, moved or not, is the caller's.  Float32 throughout, every operation
    rounded once in the written order.  exp, sin and cos are csrc/ggs_detmath.h's,
    reached through the library's ggs_detmath_eval (a device call, made only when
    something splits); ``detmath = (exp, sin, cos)`` puts other float32 array functions
    in their place, which is how a host without a device states the same event."""
    x, m, v = (np.array(a, np.float32) for a in (x, m, v))
    acc = np.asarray(acc, np.float32)
    single = x.ndim == 2
    if single:
        x, m, v, acc = x[None], m[None], v[None], acc[None]
    B, N, _ = x.shape
    prm = density_params_c(params)
    M = min(prm.max_moves, N // 2) if prm.every > 0 else 0
    pairs = np.full((B, M, 2), -1, np.int32)
    is_split = np.zeros((B, M), np.int32)
    wm, hm = _f32(max(int(W) - 1, 1)), _f32(max(int(H) - 1, 1))
    lo, hi = _f32(log_lo), _f32(log_hi)
    todo = []                                              # (b, j, d, s) of the splits
    idx = np.arange(N)
    for b in range(B if M > 0 else 0):
        alpha = x[b, :, 8]
        dead = alpha < _f32(prm.alpha_dead)
        with np.errstate(divide="ignore", invalid="ignore"):
            src = ~dead & (acc[b] / _f32(n_acc) > _f32(prm.grad_min))        # False for a NaN
        di = idx[dead]
        di = di[np.lexsort((di, alpha[di] + _f32(0.0)))]                      # ascending (alpha, index)
        si = idx[src]
        si = si[np.lexsort((si, -(acc[b][si] + _f32(0.0))))]                  # descending acc, ties to the lower index
        n = min(len(di), len(si), M)
        for j in range(n):
            d, s = int(di[j]), int(si[j])
            pairs[b, j] = (d, s)
            row = x[b, s].copy()
            L = row[2] if row[2] >= row[3] else row[3]
            if L <= _f32(prm.split_log):
                x[b, d] = row
                m[b, d] = v[b, d] = 0
            else:
                is_split[b, j] = 1
                todo.append((b, j, d, s))
    if todo:
        f_exp, f_sin, f_cos = detmath if detmath is not None else (
            lambda a: _library_detmath(0, a), lambda a: _library_detmath(2, a), lambda a: _library_detmath(3, a))
        rows = np.stack([x[b, s] for b, _, _, s in todo]).astype(np.float32)
        major_a = rows[:, 2] >= rows[:, 3]
        L = np.where(major_a, rows[:, 2], rows[:, 3]).astype(np.float32)
        sig = np.asarray(f_exp(L), np.float32)
        sn, cs = np.asarray(f_sin(rows[:, 4]), np.float32), np.asarray(f_cos(rows[:, 4]), np.float32)
        ux, uy = np.where(major_a, cs, -sn), np.where(major_a, sn, cs)
        dlt = _f32(prm.split_offset) * sig
        dx, dy = (dlt * ux) / wm, (dlt * uy) / hm
        la = np.clip(rows[:, 2] - _f32(prm.log_shrink), lo, hi)
        lb = np.clip(rows[:, 3] - _f32(prm.log_shrink), lo, hi)
        for k, (b, _, d, s) in enumerate(todo):
            for r, sign in ((s, 1), (d, -1)):
                new = rows[k].copy()
                new[0] = np.clip(rows[k, 0] + dx[k] if sign > 0 else rows[k, 0] - dx[k], _f32(0.0), _f32(1.0))
                new[1] = np.clip(rows[k, 1] + dy[k] if sign > 0 else rows[k, 1] - dy[k], _f32(0.0), _f32(1.0))
                new[2], new[3] = la[k], lb[k]
                x[b, r] = new
                m[b, r] = v[b, r] = 0
    if single:
        return x[0], m[0], v[0], pairs[0], is_split[0]
    return x, m, v, pairs, is_split


def refine(genomes, target, H: int, W: int, steps: int, *, k_sigma: float = 3.0, weight_mask=None,
           boost_only: bool = False, boost_beta: float = 1.0, lr: Optional[Sequence[float]] = None,
           beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, min_scale_splats: float = 3.0,
           max_scale_splats: float = 0.1, device: int = 0, group: Optional[int] = None, loss=None,
           background=(1.0, 1.0, 1.0), density=None) -> Dict[str, np.ndarray]:
    """``steps`` Adam steps on [B,N,9] (or [N,9]) genomes against ``target`` on the
    device → ``DeviceRefine.read``'s dict: the final state and its fitness, and per
    candidate the best state seen (``best`` / ``best_fits``), which is what a polish
    keeps.  ``lr=None``: ``DEFAULT_LR``.  A 4-D ``target`` [K,H,W,3] (``weight_mask``
    [K,H,W]) refines candidate b against image ``b // group`` in one session.
    ``loss`` (``ggs.LossParams``; default None: the fitness) descends the image loss
    L1 / MSE / SSIM of the render against ``background`` instead.
    ``density`` (a ``DensityParams``; default None: off) relocates dead splats while it
    refines; the dict then also carries ``density``, ``density_stats()``."""
    from .ga_device import DeviceRefine
    tgt = np.ascontiguousarray(target, np.float32)
    if tgt.shape[-3:] != (int(H), int(W), 3) or tgt.ndim not in (3, 4):
        raise ValueError(f"target must be [H,W,3] or [K,H,W,3] with (H, W) = {(H, W)}, got {tuple(tgt.shape)}")
    s = DeviceRefine(tgt, weight_mask, genomes, lr=DEFAULT_LR if lr is None else lr, beta1=beta1, beta2=beta2,
                     eps=eps, min_scale_splats=min_scale_splats, max_scale_splats=max_scale_splats,
                     k_sigma=k_sigma, boost_only=boost_only, boost_beta=boost_beta, device=device, group=group, loss=loss,
                     background=background)
    try:
        if density is not None:
            s.set_density(density)
        s.run(int(steps))
        out = s.read()
        if density is not None and int(DensityParams(*density).every) > 0:
            out["density"] = s.density_stats()
        return out
    finally:
        s.close()
