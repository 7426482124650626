"""Loss and gradient in one call (ggs_loss_grad*) on an MI355X: the render,
the image loss and the render's VJP composed by the library.

Reference: the float64 chain tests/_render_vjp_ref.py (render and its VJP by autograd)
with tests/_loss_ref.py's loss taken at the reference's own image.  Shapes, rows, strides
and backgrounds are the cases of tests/_render_vjp_cases.py (both layouts, white, black
and coloured backgrounds); candidate b is scored against target b of three (the
problem's target, and it flipped along either axis).  Figure of merit per row column c:
max |device - ref| over candidates and splats divided by that column's max |ref|, the
figure of tests/test_gpu_render_vjp.py, whose worst is 6.75e-6 (alpha, 600 splats).
Worst per column measured on the MI355X over all cases with the weights (0.8, 0, 0.2),
and at 48x40 with each of the four weightings:

    6.38e-7  4.75e-7  6.37e-7  5.61e-7  9.22e-7  2.59e-7  3.22e-7  3.12e-7  1.52e-6

(alpha: 1.31e-6 at 600 splats with (0.8, 0, 0.2), 1.52e-6 at 48x40 with SSIM alone); the
worst relative error of the loss: 8.22e-8.  ``BAR`` / ``LOSS_BAR`` are four times the
worst (the rule of DESIGN.md §7), under the 1e-4 ceiling.

Against ``api.fitness_grad`` in mode none, with weights (0, 1, 0) at 130x70 (axes rows,
white background, one target), the same figure measured

    1.62e-7  1.65e-7  1.19e-7  6.01e-8  2.77e-7  5.66e-8  1.04e-7  6.68e-8  1.32e-7

at worst, and the loss had the fitness's bits; ``FIT_BAR`` is four times the worst.  (The
fitness gradient takes its image from its own raster sweep; the loss reads the stored
render.)

Also: the call is bytewise the three stages called by hand, the host call bytewise the
device call, reruns and a candidate alone against the batch are bitwise equal.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import _grad_cases as cases
import _loss_ref as lref
import _render_vjp_cases as vc
import _render_vjp_ref as ref
import ggs
from ggs import api, hip

pytestmark = pytest.mark.gpu

BAR = 4 * 1.52e-6
LOSS_BAR = 4 * 8.22e-8
FIT_BAR = 4 * 2.77e-7
CEILING = 1e-4
MAIN = (0.8, 0.0, 0.2)
ALL_WEIGHTS = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), MAIN]
LAYOUT_ID = {"renderer": ggs.GGS_LAYOUT_RENDERER, "axes": ggs.GGS_LAYOUT_AXES}


@functools.lru_cache(maxsize=None)
def _targets(shape):
    t = cases.problem(shape)[1]
    out = np.ascontiguousarray(np.stack([t, t[::-1], t[:, ::-1]]))
    out.setflags(write=False)
    return out


def _ratios(dev, want):
    colmax = np.abs(want).max(axis=(0, 1))
    return np.abs(dev.astype(np.float64) - want).max(axis=(0, 1)) / colmax


def _fmt(r):
    return " ".join(f"{v:.2e}" for v in r)


def _check(case, weights):
    shape, layout, C, bg = case
    W, H, N = cases.SHAPES[shape]
    tg = _targets(shape)
    R = vc.rows(shape, layout, encode=api.encode)
    loss, grad = api.loss_grad(vc.widen(R, C), tg, H, W, weights, k_sigma=cases.K_SIGMA, background=bg, layout=layout,
                               group=1)
    assert grad.shape == (3, N, 9) and np.isfinite(grad).all() and loss.shape == (3,)
    cot, seen = lref.chain_cotangent(tg, weights, 1)
    _, want = ref.render_vjp(R, cot, H, W, cases.K_SIGMA, layout, bg)
    want_l = np.array([seen[b] for b in range(3)])
    r = _ratios(grad, want)
    rl = float(np.max(np.abs(loss - want_l) / np.abs(want_l)))
    print(f"{vc.case_id(case)} w={weights}: ratios {_fmt(r)}  loss {rl:.2e}")
    return r.max(), rl


@pytest.mark.parametrize("case", vc.CASES, ids=vc.case_id)
def test_loss_grad_against_the_float64_chain(case):
    r, rl = _check(case, MAIN)
    assert r <= BAR and rl <= LOSS_BAR
    assert BAR <= CEILING and LOSS_BAR <= CEILING


@pytest.mark.parametrize("weights", ALL_WEIGHTS[:3], ids=lambda w: "-".join(f"{v:g}" for v in w))
def test_every_weighting_against_the_float64_chain(weights):
    r, rl = _check(vc.CASES[0], weights)
    assert r <= BAR and rl <= LOSS_BAR


def _by_hand(R, tg, layout, H, W, bg, weights, group, fused):
    B, N, C = R.shape
    K = tg.shape[0]
    g, t = hip.DeviceArray.from_host(R), hip.DeviceArray.from_host(tg)
    lo, gr = hip.DeviceArray((B,)), hip.DeviceArray((B, N, 9))
    st = hip.Stream()
    lay = LAYOUT_ID[layout]
    if fused:
        api.loss_grad_device(0, st.handle, g.ptr, B, N, C, lay, t.ptr, K, group, H, W, cases.K_SIGMA, weights, lo.ptr,
                             gr.ptr, bg)
    else:
        img, cot = hip.DeviceArray((B, H, W, 3)), hip.DeviceArray((B, H, W, 3))
        api.render_layout_device(0, st.handle, g.ptr, B, N, C, lay, H, W, cases.K_SIGMA, img.ptr, bg)
        api.image_loss_device(0, st.handle, img.ptr, B, t.ptr, K, group, H, W, weights, lo.ptr, cot.ptr)
        api.render_vjp_device(0, st.handle, g.ptr, B, N, C, lay, H, W, cases.K_SIGMA, cot.ptr, gr.ptr, bg)
    st.synchronize()
    return lo.to_host(), gr.to_host()


@pytest.mark.parametrize("shape,layout,C,bg", [("130x70", "axes", 12, vc.COLOUR), ("48x40", "renderer", 9, vc.BLACK)])
def test_the_call_is_the_three_stages_by_hand(shape, layout, C, bg):
    W, H, N = cases.SHAPES[shape]
    R = vc.widen(vc.rows(shape, layout, encode=api.encode), C)
    tg = np.ascontiguousarray(_targets(shape)[:2])
    R4 = np.ascontiguousarray(np.concatenate([R, R[:1]]))            # B = 4, K = 2, group 2
    loss, grad = api.loss_grad(R4, tg, H, W, MAIN, k_sigma=cases.K_SIGMA, background=bg, layout=layout, group=2)
    for fused in (True, False):
        l, g = _by_hand(R4, tg, layout, H, W, bg, MAIN, 2, fused)
        assert l.tobytes() == loss.tobytes() and g.tobytes() == grad.tobytes(), fused
    l2, g2 = api.loss_grad(R4, tg, H, W, MAIN, k_sigma=cases.K_SIGMA, background=bg, layout=layout, group=2)
    assert l2.tobytes() == loss.tobytes() and g2.tobytes() == grad.tobytes()                # a rerun
    # the host stages: render, image_loss, render_vjp
    img = api.render(R4, H, W, k_sigma=cases.K_SIGMA, background=bg, layout=layout)
    li, cot = api.image_loss(img, tg, MAIN, group=2)
    gi = api.render_vjp(R4, cot, H, W, k_sigma=cases.K_SIGMA, background=bg, layout=layout)
    assert li.tobytes() == loss.tobytes() and gi.tobytes() == grad.tobytes()
    for b in range(4):                                                                      # alone == in the batch
        l1, g1 = api.loss_grad(R4[b:b + 1], tg[b // 2], H, W, MAIN, k_sigma=cases.K_SIGMA, background=bg,
                               layout=layout)
        assert l1[0].tobytes() == loss[b].tobytes() and g1[0].tobytes() == grad[b].tobytes(), b


def test_mse_weights_agree_with_the_fitness_gradient():
    shape = "130x70"
    W, H, N = cases.SHAPES[shape]
    G, target, _ = cases.problem(shape)
    G = np.ascontiguousarray(G)
    loss, grad = api.loss_grad(G, target, H, W, (0.0, 1.0, 0.0), k_sigma=cases.K_SIGMA, layout="axes")
    fit, want = api.fitness_grad(G, target, H, W, cases.K_SIGMA)
    r = _ratios(grad, want.astype(np.float64))
    rl = float(np.max(np.abs(loss.astype(np.float64) - fit) / fit))
    print(f"{shape}: loss_grad (0,1,0) vs fitness_grad ratios {_fmt(r)}  loss vs fitness {rl:.2e}")
    assert r.max() <= FIT_BAR and rl <= FIT_BAR and FIT_BAR <= CEILING
