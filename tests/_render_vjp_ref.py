"""Reference for the renderer's vector-Jacobian product (TEST INFRASTRUCTURE): the
chain of ``_grad_ref._candidate_loss`` restated in torch up to the clipped image,
for both row layouts and any background, so that
``torch.autograd.grad(img, g, cot)`` is the VJP.  float64 by default;
``dtype=torch.float32`` runs the same graph in single precision.

Layouts: ``"axes"`` rows are axes-angle genomes (encode.py:4-59 runs first),
``"renderer"`` rows are the renderer's x, y, log l11, log l22, l21, r, g, b, alpha
(render.py:8-47 alone).  Conventions as tests/_grad_ref.py: the
integer AABB is a constant taken from ``ggs_oracle.preprocess``, ``clip`` is
``torch.clamp``, ``max(x, eps)`` is ``where(x > eps, x, eps)``.

``render(G, ...)`` -> image float64 [B,H,W,3]; ``render_vjp(G, cot, ...)`` ->
(image [B,H,W,3], grad [B,N,9]), numpy float64.  ``cot`` is an array [B,H,W,3] or
a callable ``cot(b, img)`` that maps candidate b's detached image tensor to its
cotangent tensor (the gradient of a loss taken at that image).
"""
from __future__ import annotations

import numpy as np
import torch

import _grad_ref
import ggs_oracle as oracle
from _grad_ref import _EPS6, _EPS12, _floor_max

LAYOUTS = ("renderer", "axes")


def _bounds(G, H, W, k_sigma, layout):
    """[B] tuples of (x0, x1, y0, y1) int arrays [N]."""
    if layout == "axes":
        return _grad_ref._bounds(G, H, W, k_sigma)
    out = []
    for g in np.asarray(G, np.float32):
        p = oracle.preprocess(g, H, W, k_sigma)
        out.append(tuple(p[k].astype(np.int64) for k in oracle.BOUND_KEYS))
    return out


def _candidate_image(g, bounds, H, W, layout, background):
    """g [N,9] (dtype tensor) -> clipped image [H,W,3]."""
    dt = g.dtype
    if layout == "axes":
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
    else:
        ll11, ll22, l21, col = g[:, 2], g[:, 3], g[:, 4], g[:, 5:9]
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
    # render.py:189-196, ascending splat index
    X = torch.arange(W, dtype=dt)[None, :]
    Y = torch.arange(H, dtype=dt)[:, None]
    xi, yi = torch.arange(W)[None, :], torch.arange(H)[:, None]
    x0, x1, y0, y1 = bounds
    bg = torch.from_numpy(np.broadcast_to(np.asarray(background, np.float32), (3,)).astype(np.float64)).to(dt)
    canvas = bg.expand(H, W, 3)
    for i in range(g.shape[0]):
        inside = ((xi >= int(x0[i])) & (xi <= int(x1[i])) & (yi >= int(y0[i])) & (yi <= int(y1[i]))).to(dt)
        qx, qy = X - cx[i], Y - cy[i]
        quad = (P[i] * (qx * qx) + (2.0 * Q[i]) * (qx * qy)) + R[i] * (qy * qy)
        f = (torch.exp(-0.5 * quad) * rgba[i, 3] * inside)[..., None]
        canvas = (1.0 - f) * canvas + f * rgba[i, 0:3]
    return torch.clamp(canvas, 0.0, 1.0)


def render_vjp(G, cot, H, W, k_sigma=3.0, layout="axes", background=(1.0, 1.0, 1.0), dtype=torch.float64):
    """(image [B,H,W,3], grads): one ``cot`` gives grad [B,N,9]; a list or tuple of
    cotangents gives a list of grads from one forward pass."""
    assert layout in LAYOUTS, layout
    G = np.asarray(G, np.float32)
    if G.ndim == 2:
        G = G[None]
    many = isinstance(cot, (list, tuple))
    cots = list(cot) if many else [cot]
    bounds = _bounds(G[..., :9], H, W, k_sigma, layout)
    imgs, grads = [], [[] for _ in cots]
    for b in range(G.shape[0]):
        g = torch.from_numpy(G[b, :, :9].astype(np.float64)).to(dtype).requires_grad_(bool(cots))
        with torch.set_grad_enabled(bool(cots)):
            img = _candidate_image(g, bounds[b], H, W, layout, background)
        imgs.append(img.detach().to(torch.float64).numpy())
        for j, cj in enumerate(cots):
            v = cj(b, img.detach()) if callable(cj) else torch.from_numpy(np.asarray(cj[b], np.float64))
            (d,) = torch.autograd.grad(img, g, v.to(dtype), retain_graph=j + 1 < len(cots))
            grads[j].append(d.to(torch.float64).numpy())
    img = np.stack(imgs)
    if not cots:
        return img, None
    out = [np.stack(x) for x in grads]
    return img, (out if many else out[0])


def render(G, H, W, k_sigma=3.0, layout="axes", background=(1.0, 1.0, 1.0), dtype=torch.float64):
    return render_vjp(G, [], H, W, k_sigma, layout, background, dtype)[0]
