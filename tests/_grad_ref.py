"""Reference for the fitness gradient (TEST INFRASTRUCTURE): the chain
encode -> preprocess -> "over" blend -> clip -> fitness of oracle/ggs_oracle.py
restated in torch, so that autograd differentiates it.  float64 by default;
``dtype=torch.float32`` runs the same graph in single precision.

Conventions:

* the integer AABB is a constant: a 0/1 mask built from ``ggs_oracle.preprocess``'s
  integer bounds (the only thing this module takes from the oracle);
* ``clip(x, lo, hi)`` is ``torch.clamp`` (gradient passes iff lo <= x <= hi);
* ``max(x, eps)`` is ``where(x > eps, x, eps)`` (gradient passes iff x > eps).

``loss(G, ...)`` -> float64 [B]; ``loss_and_grad(G, ...)`` -> (loss [B], grad [B,N,9]),
both numpy float64.  ``bounds_from``: genomes the AABBs are taken from (default: G
itself) — finite differences perturb G and keep the bounds.
"""
from __future__ import annotations

import numpy as np
import torch

import ggs_oracle as oracle
from detmath import EPS6, EPS12

_EPS6, _EPS12 = float(EPS6), float(EPS12)


def _bounds(G, H, W, k_sigma):
    """[B] lists of (x0, x1, y0, y1) int arrays [N]."""
    out = []
    for g in np.asarray(G, np.float32):
        p = oracle.preprocess(oracle.genome_to_renderer(g), H, W, k_sigma)
        out.append(tuple(p[k].astype(np.int64) for k in oracle.BOUND_KEYS))
    return out


def _floor_max(x, eps):
    return torch.where(x > eps, x, torch.full_like(x, eps))


def _candidate_loss(g, bounds, target, omega, D, H, W):
    """g [N,9] (dtype tensor) -> scalar loss."""
    dt = g.dtype
    # encode.py:4-59
    sx, sy = torch.exp(g[:, 2]), torch.exp(g[:, 3])
    s, c = torch.sin(g[:, 4]), torch.cos(g[:, 4])
    sx2, sy2, c2, s2 = sx * sx, sy * sy, c * c, s * s
    vxx = sx2 * c2 + sy2 * s2
    vxy = ((sx2 - sy2) * s) * c
    vyy = sx2 * s2 + sy2 * c2
    l11 = torch.sqrt(_floor_max(vxx, _EPS12))
    l21 = vxy / l11
    l22 = torch.sqrt(_floor_max(vyy - l21 * l21, _EPS12))
    ll11, ll22 = torch.log(l11), torch.log(l22)
    col = torch.clamp(g[:, 5:9], 0.0, 255.0)
    # render.py:8-47
    cx = torch.clamp(g[:, 0], 0.0, 1.0) * float(W - 1)
    cy = torch.clamp(g[:, 1], 0.0, 1.0) * float(H - 1)
    p11 = _floor_max(torch.exp(ll11), _EPS6)
    p22 = _floor_max(torch.exp(ll22), _EPS6)
    i11, i22 = 1.0 / p11, 1.0 / p22
    i21 = (-l21) * (i11 * i22)
    P = i11 * i11 + i21 * i21
    Q = i21 * i22
    R = i22 * i22
    rgba = torch.clamp(col, 0.0, 255.0) / 255.0
    # render.py:189-196, ascending splat index, white background (fitness.py:15)
    X = torch.arange(W, dtype=dt)[None, :]
    Y = torch.arange(H, dtype=dt)[:, None]
    xi, yi = torch.arange(W)[None, :], torch.arange(H)[:, None]
    x0, x1, y0, y1 = bounds
    canvas = torch.ones((H, W, 3), dtype=dt)
    for i in range(g.shape[0]):
        inside = ((xi >= int(x0[i])) & (xi <= int(x1[i])) & (yi >= int(y0[i])) & (yi <= int(y1[i]))).to(dt)
        qx, qy = X - cx[i], Y - cy[i]
        quad = (P[i] * (qx * qx) + (2.0 * Q[i]) * (qx * qy)) + R[i] * (qy * qy)
        f = (torch.exp(-0.5 * quad) * rgba[i, 3] * inside)[..., None]
        canvas = (1.0 - f) * canvas + f * rgba[i, 0:3]
    img = torch.clamp(canvas, 0.0, 1.0)
    return (omega[..., None] * (img - target) ** 2).sum() / D


def _weights(H, W, weight_mask, boost_only, boost_beta, dt):
    """(omega [H,W], D) of fitness.py:16-31."""
    if weight_mask is None:
        return torch.ones((H, W), dtype=dt), 3.0 * H * W
    w = np.asarray(weight_mask, np.float32)
    if boost_only:
        wb = np.float32(1.0) + np.float32(boost_beta) * np.clip(w, np.float32(0), np.float32(1))
        return torch.from_numpy(wb.astype(np.float64)).to(dt), 3.0 * H * W * (wb.astype(np.float64).mean() + 1e-12)
    return torch.from_numpy(w.astype(np.float64)).to(dt), float(w.astype(np.float64).sum()) + 1e-12


def loss_and_grad(G, target, H, W, k_sigma=3.0, weight_mask=None, boost_only=False, boost_beta=1.0,
                  dtype=torch.float64, bounds_from=None, need_grad=True):
    G = np.asarray(G, np.float32)
    if G.ndim == 2:
        G = G[None]
    bounds = _bounds(G if bounds_from is None else bounds_from, H, W, k_sigma)
    tgt = torch.from_numpy(np.asarray(target, np.float32).astype(np.float64)).to(dtype)
    omega, D = _weights(H, W, weight_mask, boost_only, boost_beta, dtype)
    losses, grads = [], []
    for b in range(G.shape[0]):
        g = torch.from_numpy(G[b, :, :9].astype(np.float64)).to(dtype).requires_grad_(need_grad)
        with torch.set_grad_enabled(need_grad):
            L = _candidate_loss(g, bounds[b], tgt, omega, D, H, W)
        losses.append(float(L.detach()))
        if need_grad:
            L.backward()
            grads.append(g.grad.detach().to(torch.float64).numpy())
    losses = np.asarray(losses, np.float64)
    return (losses, np.stack(grads)) if need_grad else losses


def loss(G, target, H, W, k_sigma=3.0, weight_mask=None, boost_only=False, boost_beta=1.0,
         dtype=torch.float64, bounds_from=None):
    return loss_and_grad(G, target, H, W, k_sigma, weight_mask, boost_only, boost_beta, dtype, bounds_from,
                         need_grad=False)


def loss_f64(G64, bounds_from, target, H, W, k_sigma=3.0, weight_mask=None, boost_only=False, boost_beta=1.0):
    """The loss of ONE candidate at float64 genes G64 [N,9] (finite differences step
    below float32 resolution), AABBs from the float32 genomes ``bounds_from`` [N,9]."""
    bounds = _bounds(np.asarray(bounds_from, np.float32)[None], H, W, k_sigma)[0]
    tgt = torch.from_numpy(np.asarray(target, np.float32).astype(np.float64))
    omega, D = _weights(H, W, weight_mask, boost_only, boost_beta, torch.float64)
    with torch.no_grad():
        return float(_candidate_loss(torch.from_numpy(np.asarray(G64, np.float64)), bounds, tgt, omega, D, H, W))
