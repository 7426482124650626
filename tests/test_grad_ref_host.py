"""tests/_grad_ref.py pinned on the CPU, before any GPU result is compared with it:

* its float64 loss is ``oracle.fitness_many`` (1e-6 relative) in the three modes;
* its autograd gradient is the float64 central difference (1e-5 relative) on
  entries away from clip boundaries, the AABBs held fixed;
* where alpha is exactly 255 the clip passes the gradient on one side only, so the
  central difference is half the autograd value (the inclusive-boundary rule).
"""
from __future__ import annotations

import numpy as np
import pytest

import _grad_cases as cases
import _grad_ref
import ggs_oracle as oracle

SHAPE = "48x40"
# perturbation per column: a fraction of the column's scale, far above float64 noise
STEP = (1e-6, 1e-6, 1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4, 1e-4)


@pytest.mark.parametrize("mode", cases.MODES)
def test_loss_is_the_oracles(mode):
    W, H, N = cases.SHAPES[SHAPE]
    G, target, mask = cases.problem(SHAPE)
    kw = cases.mode_kwargs(mode, mask)
    want = oracle.fitness_many(list(G), target, H, W, cases.K_SIGMA, **kw)
    got, _ = cases.reference(SHAPE, mode)
    rel = np.abs(got - want) / np.abs(want)
    print("relative loss difference", rel)
    assert rel.max() < 1e-6


def _central(G, b, s, c, target, H, W, kw):
    g0 = G[b].astype(np.float64)
    h = STEP[c]
    out = []
    for sign in (+1.0, -1.0):
        g = g0.copy()
        g[s, c] += sign * h
        out.append(_grad_ref.loss_f64(g, G[b], target, H, W, cases.K_SIGMA, **kw))
    return (out[0] - out[1]) / (2.0 * h)


def test_gradient_is_the_central_difference():
    W, H, N = cases.SHAPES[SHAPE]
    G, target, mask = cases.problem(SHAPE)
    kw = cases.mode_kwargs("weighted", mask)
    _, grad = cases.reference(SHAPE, "weighted")
    rng = np.random.default_rng(3)
    colmax = np.abs(grad).max(axis=(0, 1))
    checked = 0
    for c in range(9):
        # two entries per column that carry a real gradient and sit inside their clip range
        order = rng.permutation(3 * N)
        n_col = 0
        for k in order:
            b, s = divmod(int(k), N)
            x = float(G[b, s, c])
            lo, hi = ((0.0, 1.0) if c < 2 else (0.0, 255.0) if c >= 5 else (-np.inf, np.inf))
            if not (lo + 10 * STEP[c] < x < hi - 10 * STEP[c]) or abs(grad[b, s, c]) < 1e-3 * colmax[c]:
                continue
            fd = _central(G, b, s, c, target, H, W, kw)
            rel = abs(fd - grad[b, s, c]) / abs(grad[b, s, c])
            print(f"col {c} cand {b} splat {s}: autograd {grad[b, s, c]:.6e} central {fd:.6e} rel {rel:.2e}")
            assert rel < 1e-5
            n_col += 1
            checked += 1
            if n_col == 2:
                break
    assert checked == 18


def test_alpha_255_takes_the_inclusive_side():
    W, H, N = cases.SHAPES[SHAPE]
    G, target, mask = cases.problem(SHAPE)
    kw = cases.mode_kwargs("weighted", mask)
    _, grad = cases.reference(SHAPE, "weighted")
    s = cases.planted_index("opaque", N)
    assert G[0, s, 8] == 255.0 and grad[0, s, 8] != 0.0
    fd = _central(G, 0, s, 8, target, H, W, kw)
    print("alpha = 255: autograd", grad[0, s, 8], "central difference", fd)
    assert abs(fd - 0.5 * grad[0, s, 8]) < 1e-5 * abs(0.5 * grad[0, s, 8])


def test_clipped_columns_have_zero_gradient():
    W, H, N = cases.SHAPES[SHAPE]
    _, grad = cases.reference(SHAPE, "none")
    s = cases.planted_index("clipped", N)
    assert grad[0, s, 0] == 0.0 and grad[0, s, 5] == 0.0
    assert np.abs(grad[0, s, 6:9]).max() > 0.0
