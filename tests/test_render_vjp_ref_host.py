"""tests/_render_vjp_ref.py pinned twice on the CPU.

1. Its image against ``oracle.render`` (float32 operations in the reference's
   order), both layouts, white and coloured background.  Measured max |ref - oracle|
   over the cases below: 4.70e-7 (130x70, renderer rows, white); ``IMAGE_BAR`` is four
   times that.  (The
   project's image bar, 1e-4, is the ceiling above which a figure would be a defect;
   tests/_grad_ref.py is pinned to ``oracle.fitness_many`` at 4e-8 the same way.)
2. With the cotangent d fitness / d img of the three fitness modes, taken by autograd
   at ``img.detach()``, its VJP against ``_grad_ref.loss_and_grad``'s gradient.  Both
   are float64 autograd over the same operations and differ by summation order only.
   Figure: max |vjp - grad| / max |grad| per genome column; measured worst over the
   cases below: 0 in every column (the two graphs run the same torch operations in the
   same order, so even the sums agree bit for bit); ``VJP_BAR`` is four times that,
   i.e. equality.  A ratio above 1e-9 would mean the two graphs differ.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _grad_cases as cases
import _grad_ref
import _render_vjp_cases as vc
import _render_vjp_ref as ref
import ggs_oracle as oracle

MEASURED_IMAGE = 4.70e-7
IMAGE_BAR = 4 * MEASURED_IMAGE
MEASURED_VJP = 0.0
VJP_BAR = 4 * MEASURED_VJP


@pytest.mark.parametrize("layout", ref.LAYOUTS)
@pytest.mark.parametrize("bg", [vc.WHITE, vc.COLOUR], ids=["white", "colour"])
@pytest.mark.parametrize("shape", ["48x40", "130x70"])
def test_image_is_the_oracle_render(shape, bg, layout):
    W, H, N = cases.SHAPES[shape]
    R = vc.rows(shape, layout)
    img = ref.render(R, H, W, cases.K_SIGMA, layout, bg)
    want = oracle.render(R if layout == "renderer" else oracle.genome_to_renderer_batched(R), H, W,
                         k_sigma=cases.K_SIGMA, background=bg)
    err = float(np.abs(img - want.astype(np.float64)).max())
    print(f"{shape} {layout} bg={bg}: image max|ref - oracle| = {err:.3e}")
    assert img.shape == (3, H, W, 3) and err <= IMAGE_BAR


@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("shape", ["48x40", "130x70"])
def test_vjp_of_the_fitness_cotangent_is_the_fitness_gradient(shape, mode):
    W, H, N = cases.SHAPES[shape]
    G, target, mask = cases.problem(shape)
    _, want = cases.reference(shape, mode)
    omega, D = _grad_ref._weights(H, W, **cases.mode_kwargs(mode, mask), dt=torch.float64)
    tgt = torch.from_numpy(np.asarray(target, np.float64))

    def cot(b, img):
        x = img.clone().requires_grad_(True)
        L = (omega[..., None] * (x - tgt) ** 2).sum() / D
        return torch.autograd.grad(L, x)[0]

    _, got = ref.render_vjp(G, cot, H, W, cases.K_SIGMA, "axes", vc.WHITE)
    r = np.abs(got - want).max(axis=(0, 1)) / np.abs(want).max(axis=(0, 1))
    print(f"{shape} {mode}: vjp vs loss_and_grad ratios " + " ".join(f"{v:.2e}" for v in r))
    assert r.max() <= VJP_BAR
