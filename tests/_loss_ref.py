"""Reference for the image loss (TEST INFRASTRUCTURE): the definition
in torch on the CPU, float64 by default, with ``torch.autograd.grad`` for the cotangent.

    loss[b] = w_l1 mean|x - y| + w_mse mean (x - y)^2 + w_ssim (1 - mean SSIM(x, y))

for x = img[b] and y = targets[b // group], the means over all 3 H W values.  SSIM per
channel as the common 3DGS ``ssim()`` computes it: the 11 x 11 window is the outer
product of the 1-D taps exp(-(i - 5)^2 / 4.5) normalised to sum 1 (float64), applied
with ``conv2d(padding=5)`` (zero padding), C1 = 0.01^2, C2 = 0.03^2,
SSIM = ((2 mux muy + C1)(2 sxy + C2)) / ((mux^2 + muy^2 + C1)(sxx + syy + C2)) with
sxx = E[x^2] - mux^2 and so on.  ``dtype=torch.float32`` runs the same graph in single
precision (the yardstick the float64 device path is measured beside).

``analytic_cot`` restates d (Sum m) / d x without autograd, from the partials of m at a
window centre with the variances held fixed (the formula the kernel uses):
    d(Sum m)/dx_p = conv(a)_p + 2 x_p conv(dsxx)_p + y_p conv(dsxy)_p,
    a = dmu - 2 mux dsxx - muy dsxy.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

RADIUS = 5
C1, C2 = 0.01 ** 2, 0.03 ** 2


def taps(dtype=torch.float64) -> torch.Tensor:
    i = torch.arange(2 * RADIUS + 1, dtype=torch.float64) - RADIUS
    g = torch.exp(-(i * i) / 4.5)
    return (g / g.sum()).to(dtype)


def _window(dtype) -> torch.Tensor:
    g = taps(torch.float64)
    return (g[:, None] * g[None, :]).to(dtype)[None, None].expand(3, 1, -1, -1).contiguous()


def _conv(z: torch.Tensor) -> torch.Tensor:
    """z [3,H,W] -> the zero-padded window mean per channel."""
    return F.conv2d(z[None], _window(z.dtype), padding=RADIUS, groups=3)[0]


def ssim_map(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """x, y [H,W,3] -> m [3,H,W]."""
    xc, yc = x.permute(2, 0, 1), y.permute(2, 0, 1)
    mux, muy = _conv(xc), _conv(yc)
    sxx = _conv(xc * xc) - mux * mux
    syy = _conv(yc * yc) - muy * muy
    sxy = _conv(xc * yc) - mux * muy
    return ((2 * mux * muy + C1) * (2 * sxy + C2)) / ((mux * mux + muy * muy + C1) * (sxx + syy + C2))


def loss_tensor(x: torch.Tensor, y: torch.Tensor, weights) -> torch.Tensor:
    """The scalar loss of one image x [H,W,3] against y (a differentiable torch graph)."""
    w_l1, w_mse, w_ssim = (float(v) for v in weights)
    d = x - y
    out = x.new_zeros(())
    if w_l1:
        out = out + w_l1 * d.abs().mean()
    if w_mse:
        out = out + w_mse * (d * d).mean()
    if w_ssim:
        out = out + w_ssim * (1.0 - ssim_map(x, y).mean())
    return out


def image_loss(img, targets, weights, group=None, dtype=torch.float64):
    """(loss [B], cot [B,H,W,3]) as float64 numpy arrays; targets [K,H,W,3] or [H,W,3]."""
    img = np.asarray(img, np.float32)
    tg = np.asarray(targets, np.float32)
    B = img.shape[0]
    if tg.ndim == 3:
        tg, group = tg[None], B
    if group is None:
        group = max(B // tg.shape[0], 1)
    losses, cots = [], []
    for b in range(B):
        x = torch.from_numpy(img[b].astype(np.float64)).to(dtype).requires_grad_(True)
        y = torch.from_numpy(tg[b // group].astype(np.float64)).to(dtype)
        L = loss_tensor(x, y, weights)
        (g,) = torch.autograd.grad(L, x)
        losses.append(float(L.detach().to(torch.float64)))
        cots.append(g.to(torch.float64).numpy())
    return np.asarray(losses, np.float64), np.stack(cots)


def chain_cotangent(targets, weights, group):
    """For ``_render_vjp_ref.render_vjp``: cot(b, img) = d loss / d img at the reference's
    own image of candidate b (float64), and the losses it saw, by candidate."""
    tg = np.asarray(targets, np.float32)
    seen = {}

    def cot(b, im):
        x = im.detach().to(torch.float64).clone().requires_grad_(True)
        y = torch.from_numpy(tg[b // group].astype(np.float64))
        L = loss_tensor(x, y, weights)
        (g,) = torch.autograd.grad(L, x)
        seen[b] = float(L.detach())
        return g

    return cot, seen


def _conv_np(z: np.ndarray) -> np.ndarray:
    return _conv(torch.from_numpy(np.ascontiguousarray(z, np.float64))).numpy()


def analytic_cot(x, y, weights) -> np.ndarray:
    """d loss / d x [H,W,3] of one image by the three-map formula, float64 numpy."""
    w_l1, w_mse, w_ssim = (float(v) for v in weights)
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    n = x.size
    d = x - y
    out = (w_l1 * np.sign(d) + 2.0 * w_mse * d) / n
    if w_ssim:
        xc, yc = x.transpose(2, 0, 1), y.transpose(2, 0, 1)
        mux, muy = _conv_np(xc), _conv_np(yc)
        sxx = _conv_np(xc * xc) - mux * mux
        syy = _conv_np(yc * yc) - muy * muy
        sxy = _conv_np(xc * yc) - mux * muy
        A1, A2 = 2 * mux * muy + C1, 2 * sxy + C2
        B1, B2 = mux * mux + muy * muy + C1, sxx + syy + C2
        dmu = 2 * A2 * (muy * B1 - mux * A1) / (B1 * B1 * B2)
        dsxx = -A1 * A2 / (B1 * B2 * B2)
        dsxy = 2 * A1 / (B1 * B2)
        a = dmu - 2 * mux * dsxx - muy * dsxy
        g = _conv_np(a) + 2 * xc * _conv_np(dsxx) + yc * _conv_np(dsxy)
        out = out - (w_ssim / n) * g.transpose(1, 2, 0)
    return out
