"""The fitness gradient (ggs_fitness_grad*, csrc/ggs_grad.hip) on an MI355X against
the float64 autograd reference tests/_grad_ref.py.

Figure of merit, per case and genome column c: max |device - ref| over the three
candidates and all splats, divided by that column's max |ref|.  The same graph in
float32 on the CPU gives at most 7e-7; the device sums in another order.  Worst
ratio per column measured on the MI355X over all cases below (x, y, log a, log b,
theta, r, g, b, alpha):

    6.11e-7  4.71e-7  3.47e-7  2.56e-7  6.09e-7  2.94e-7  3.76e-7  3.97e-7  5.85e-7

(the f = 1 row alone: at most 1.92e-7).

``BAR`` is four times the worst of these (the rule DESIGN.md §7 uses for the
Box-Muller normals); 1e-4, the project's image bar, is the ceiling above which a
figure is a defect.  The planted f = 1 row (alpha 255, centre on a pixel: the
backward's exact walk) is held to the same bar.

Also: the fitness beside the gradient has ggs_fitness_device's bits, reruns are
bitwise equal, candidate b of a batch is bitwise the candidate alone, and the
host-pointer call is bitwise the device-pointer call.
"""
from __future__ import annotations

import numpy as np
import pytest

import _grad_cases as cases
import ggs
from ggs import api, hip

pytestmark = pytest.mark.gpu

BAR = 4 * 6.11e-7
# shape, mode, genome stride
CASES = [("48x40", "none", 9), ("48x40", "weighted", 12), ("48x40", "boost", 9),
         ("64x128", "weighted", 9), ("64x128", "boost", 12),
         ("130x70", "none", 12), ("130x70", "weighted", 9), ("130x70", "boost", 9),
         ("n600", "weighted", 9)]


def _widen(G, C):
    if C == 9:
        return np.ascontiguousarray(G)
    out = np.full(G.shape[:2] + (C,), 123.0, np.float32)       # the extra columns are never read
    out[..., :9] = G
    return out


def _mode_id(mode):
    return {"none": ggs.GGS_FIT_NONE, "weighted": ggs.GGS_FIT_WEIGHTED, "boost": ggs.GGS_FIT_BOOST}[mode]


def _device_call(G, target, mask, mode, beta, H, W, with_out=True):
    B, N, C = G.shape
    g, t = hip.DeviceArray.from_host(G), hip.DeviceArray.from_host(target)
    m = hip.DeviceArray.from_host(mask) if mode != ggs.GGS_FIT_NONE else None
    o, d = hip.DeviceArray((B,)), hip.DeviceArray((B, N, 9))
    st = hip.Stream()
    api.fitness_grad_device(0, st.handle, g.ptr, B, N, C, t.ptr, m.ptr if m else 0, mode, beta, H, W, cases.K_SIGMA,
                            o.ptr if with_out else 0, d.ptr)
    st.synchronize()
    return o.to_host(), d.to_host()


def _ratios(dev, ref):
    colmax = np.abs(ref).max(axis=(0, 1))
    return np.abs(dev.astype(np.float64) - ref).max(axis=(0, 1)) / colmax


@pytest.mark.parametrize("shape,mode,C", CASES)
def test_gradient_against_float64_autograd(shape, mode, C):
    W, H, N = cases.SHAPES[shape]
    G, target, mask = cases.problem(shape)
    kw = cases.mode_kwargs(mode, mask)
    _, ref = cases.reference(shape, mode)
    fit, grad = api.fitness_grad(_widen(G, C), target, H, W, cases.K_SIGMA, **kw)
    assert grad.shape == (3, N, 9) and np.isfinite(grad).all()
    r = _ratios(grad, ref)
    print(f"{shape} {mode} C={C}: ratios " + " ".join(f"{v:.2e}" for v in r))
    s = cases.planted_index("opaque", N)
    colmax = np.abs(ref).max(axis=(0, 1))
    r1 = np.abs(grad[0, s].astype(np.float64) - ref[0, s]) / colmax
    print(f"{shape} {mode} C={C}: f = 1 row " + " ".join(f"{v:.2e}" for v in r1))
    assert r.max() <= BAR
    assert r1.max() <= BAR
    # the clip rule: x < 0 and red > 255 get exactly zero
    s = cases.planted_index("clipped", N)
    assert grad[0, s, 0] == 0.0 and grad[0, s, 5] == 0.0
    # the fitness beside it is the fitness path's
    assert fit.tobytes() == api.fitness(_widen(G, C), target, H, W, cases.K_SIGMA, **kw).tobytes()


@pytest.mark.parametrize("shape,mode", [("130x70", "weighted"), ("n600", "boost")])
def test_bits_do_not_depend_on_the_call(shape, mode):
    W, H, N = cases.SHAPES[shape]
    G, target, mask = cases.problem(shape)
    G = np.ascontiguousarray(G)
    kw = cases.mode_kwargs(mode, mask)
    mid, beta = _mode_id(mode), kw["boost_beta"]
    fit, grad = api.fitness_grad(G, target, H, W, cases.K_SIGMA, **kw)
    fit2, grad2 = api.fitness_grad(G, target, H, W, cases.K_SIGMA, **kw)
    assert grad.tobytes() == grad2.tobytes() and fit.tobytes() == fit2.tobytes()          # a rerun
    dfit, dgrad = _device_call(G, target, mask, mid, beta, H, W)
    assert dgrad.tobytes() == grad.tobytes() and dfit.tobytes() == fit.tobytes()          # host == device call
    _, dgrad0 = _device_call(G, target, mask, mid, beta, H, W, with_out=False)           # out may be NULL
    assert dgrad0.tobytes() == grad.tobytes()
    # the fitness is ggs_fitness_device's
    g, t, m = hip.DeviceArray.from_host(G), hip.DeviceArray.from_host(target), hip.DeviceArray.from_host(mask)
    o = hip.DeviceArray((3,))
    st = hip.Stream()
    api.fitness_device(0, st.handle, g.ptr, 3, N, 9, t.ptr, m.ptr, mid, beta, H, W, cases.K_SIGMA, o.ptr)
    st.synchronize()
    assert o.to_host().tobytes() == fit.tobytes()
    for b in range(3):                                                                    # alone == in the batch
        f1, g1 = api.fitness_grad(G[b:b + 1], target, H, W, cases.K_SIGMA, **kw)
        assert g1[0].tobytes() == grad[b].tobytes() and f1[0] == fit[b]


def test_workspace_budget_is_reported():
    # 2048 x 2048 with 4096 splats: one candidate's strip partials are far above the budget
    G = np.zeros((1, 4096, 9), np.float32)
    with pytest.raises(ggs.GGSError, match="budget"):
        api.fitness_grad(G, np.zeros((2048, 2048, 3), np.float32), 2048, 2048)
