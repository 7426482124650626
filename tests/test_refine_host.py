"""ggs.refine.adam_step, the numpy statement the device refiner is held to: against
an independent float64 Adam within float32 rounding, the clamp and the wrap, the
first step, and a zero learning rate."""
from __future__ import annotations

import numpy as np
import pytest

from ggs import ga
from ggs.refine import DEFAULT_LR, AdamParams, adam_step, bias_corrections

LO, HI = ga.scale_log_bounds(64, 64, 0.5, 0.5)


def _state(seed, n=40):
    rng = np.random.default_rng(seed)
    x = np.concatenate([rng.uniform(0.05, 0.95, (n, 2)), rng.uniform(LO + 0.3, HI - 0.3, (n, 2)),
                        rng.uniform(-3.0, 3.0, (n, 1)), rng.uniform(5, 250, (n, 4))], axis=1).astype(np.float32)
    g = (rng.normal(0, 1, (n, 9)) * 10.0 ** rng.uniform(-6, -2, (n, 9))).astype(np.float32)
    m = (rng.normal(0, 1e-3, (n, 9))).astype(np.float32)
    v = (rng.uniform(0, 1e-5, (n, 9))).astype(np.float32)
    return x, g, m, v


def _adam64(x, g, m, v, t, p):
    x, g, m, v = (a.astype(np.float64) for a in (x, g, m, v))
    b1, b2 = float(np.float32(p.beta1)), float(np.float32(p.beta2))
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    step = np.asarray(p.lr, np.float32).astype(np.float64) * (m / (1 - b1 ** t)) / (
        np.sqrt(v / (1 - b2 ** t)) + float(np.float32(p.eps)))
    return x - step, m, v, step


@pytest.mark.parametrize("t", [1, 2, 37, 5000])
def test_against_float64_adam(t):
    p = AdamParams(lr=DEFAULT_LR, log_lo=LO, log_hi=HI)
    x, g, m, v = _state(t)
    if t == 1:
        m[:], v[:] = 0.0, 0.0
    x1, m1, v1 = adam_step(x, g, m, v, t, p)
    assert x1.dtype == m1.dtype == v1.dtype == np.float32
    x64, m64, v64, step = _adam64(x, g, m, v, t, p)
    eps32 = np.finfo(np.float32).eps
    assert np.abs(m1 - m64).max() <= 4 * eps32 * np.abs(m64).max()
    assert np.abs(v1 - v64).max() <= 4 * eps32 * np.abs(v64).max()
    # a handful of float32 roundings on the step, one on x (the state above stays inside every clamp)
    tol = 16 * eps32 * np.abs(step) + eps32 * np.abs(x64)
    assert (np.abs(x1 - x64) <= tol).all()
    if t == 1:          # m / (1 - beta1) = g, sqrt(v / (1 - beta2)) = |g|: a full step of lr against the sign
        big = np.abs(g) > 1e-4
        want = x - np.asarray(p.lr, np.float32) * np.sign(g)
        assert np.allclose(x1[big], want[big], rtol=1e-3, atol=0)


def test_bias_corrections_are_float64_then_rounded_once():
    c1, c2 = bias_corrections(0.9, 0.999, 3)
    assert c1 == np.float32(1.0 - float(np.float32(0.9)) ** 3) and c2 == np.float32(1.0 - float(np.float32(0.999)) ** 3)
    assert c1.dtype == np.float32


def test_clamp_and_wrap_are_applied():
    p = AdamParams(lr=(1.0,) * 5 + (500.0,) * 4, log_lo=LO, log_hi=HI)
    x = np.array([[0.5, 0.5, HI - 0.1, LO + 0.1, 3.0, 250.0, 5.0, 128.0, 128.0]], np.float32)
    g = np.array([[-1, 1, -1, 1, -1, -1, 1, 1e-30, 0]], np.float32) * np.float32(1e-3)
    z = np.zeros_like(x)
    x1, _, _ = adam_step(x, g, z, z, 1, p)
    assert x1[0, 0] == 1.0 and x1[0, 1] == 0.0
    assert x1[0, 2] == HI and x1[0, 3] == LO
    assert -np.pi <= x1[0, 4] < np.pi and abs(x1[0, 4] - (4.0 - 2 * np.pi)) < 1e-4     # 3 + 1 wrapped once
    # (the step is 1 / (1 + eps / |g|) = 1 - 1e-5 of lr)
    assert x1[0, 5] == 255.0 and x1[0, 6] == 0.0
    assert x1[0, 8] == 128.0                                                              # zero gradient: no step


def test_zero_learning_rate_keeps_every_bit():
    p = AdamParams(lr=(0.0,) * 9, log_lo=LO, log_hi=HI)
    x, g, m, v = _state(11)
    x[0, 4], x[1, 4] = -ga.PI32, np.nextafter(ga.PI32, np.float32(0))
    x1, m1, v1 = adam_step(x, g, m, v, 5, p)
    assert x1.tobytes() == x.tobytes()
    assert m1.tobytes() != m.tobytes() and v1.tobytes() != v.tobytes()


def test_step_numbers_start_at_one():
    x, g, m, v = _state(1)
    with pytest.raises(ValueError):
        adam_step(x, g, m, v, 0, AdamParams())
