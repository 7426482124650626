"""The device Adam refiner (ggs_refine_*, ga_device.DeviceRefine) on an MI355X:

* one step is ``ggs.refine.adam_step`` bit for bit on the gradient the step used;
* 50 steps towards a render of a perturbed copy of the start: the best so far
  never rises and ends strictly below where it began;
* candidate b of a four-candidate session is bitwise the candidate alone;
* ``genetic_approx(polish_steps=20)`` is no worse than ``polish_steps=0``.
"""
from __future__ import annotations

import numpy as np
import pytest

import ggs_oracle as oracle
from ggs import api, ga
from ggs.ga_device import DeviceRefine
from ggs.refine import DEFAULT_LR, AdamParams, adam_step

pytestmark = pytest.mark.gpu
H = W = 64
N = 16
MIN_S, MAX_S = 0.5, 0.5


def _problem(B, seed=3):
    G = oracle.synthetic_population(B, N, H, W, seed=seed)
    rng = np.random.default_rng(seed)
    moved = G[0].copy()
    moved[:, 0:2] = np.clip(moved[:, 0:2] + rng.normal(0, 0.03, (N, 2)), 0, 1)
    moved[:, 5:8] = np.clip(moved[:, 5:8] + rng.normal(0, 20, (N, 3)), 0, 255)
    target = oracle.render(oracle.genome_to_renderer_batched(moved[None]), H, W, k_sigma=3.0)[0]
    mask = rng.uniform(0.2, 1.0, (H, W)).astype(np.float32)
    return ga.clamp_genome(G, H, W, MIN_S, MAX_S), target, mask


def _session(G, target, mask, **kw):
    return DeviceRefine(target, mask, G, lr=DEFAULT_LR, min_scale_splats=MIN_S, max_scale_splats=MAX_S, **kw)


def test_a_step_is_adam_step_bit_for_bit():
    G, target, mask = _problem(3)
    lo, hi = ga.scale_log_bounds(H, W, MIN_S, MAX_S)
    p = AdamParams(lr=DEFAULT_LR, log_lo=lo, log_hi=hi)
    s = _session(G, target, mask)
    x = s.read()["genomes"]
    assert x.tobytes() == G.tobytes()
    m, v = np.zeros_like(x), np.zeros_like(x)
    for t in (1, 2, 3):
        s.run(1)
        r = s.read()
        # the gradient of the step is the gradient call's, the fitness the fitness call's
        fit, grad = api.fitness_grad(x, target, H, W, 3.0, weight_mask=mask)
        assert r["last_grad"].tobytes() == grad.tobytes()
        x, m, v = adam_step(x, r["last_grad"], m, v, t, p)
        assert r["genomes"].tobytes() == x.tobytes(), t
        assert r["fitness"].tobytes() == api.fitness(x, target, H, W, 3.0, weight_mask=mask).tobytes()
    s.close()


def test_fifty_steps_improve_and_best_never_rises():
    G, target, mask = _problem(3)
    s = _session(G, target, mask)
    first = s.read()["best_fits"].copy()
    assert first.tobytes() == api.fitness(G, target, H, W, 3.0, weight_mask=mask).tobytes()
    prev = first
    for _ in range(5):
        s.run(10)
        r = s.read()
        assert (r["best_fits"] <= prev).all()
        prev = r["best_fits"].copy()
    print("best fitness", first, "->", prev)
    assert (prev < first).all()
    # the best individual's fitness is what the session says
    assert api.fitness(r["best"], target, H, W, 3.0, weight_mask=mask).tobytes() == prev.tobytes()
    s.close()


def test_a_candidate_does_not_depend_on_its_session():
    G, target, mask = _problem(4)
    s = _session(G, target, None)
    s.run(6)
    r4 = s.read()
    s.close()
    for b in (0, 3):
        s = _session(G[b:b + 1], target, None)
        s.run(6)
        r1 = s.read()
        s.close()
        for k in ("genomes", "fitness", "best", "best_fits", "last_grad"):
            assert r1[k][0].tobytes() == r4[k][b].tobytes(), (b, k)


def test_polish_is_no_worse():
    rng = np.random.default_rng(5)
    img = (rng.uniform(0, 255, (32, 32, 3))).astype(np.uint8)
    zero = dict.fromkeys(("xy", "alog", "blog", "theta", "rgb", "alpha"), 0.0)
    smax = dict(xy=0.05, alog=0.2, blog=0.2, theta=0.3, rgb=20.0, alpha=20.0)
    kw = dict(pop_size=8, n_splats=12, generations=4, tour_k=2, elite_k=1, cxpb=0.5, mutpb=0.3,
              mut_sigma_max=smax, mut_sigma_min=zero, schedule="linear", min_scale_splats=MIN_S,
              max_scale_splats=MAX_S, k_sigma=3.0, mask_strength=0.5, boost_only=False, seed=9,
              progress=False, backend="device")
    _, f0 = ga.genetic_approx(img, 48, 48, None, **kw)
    best, f1 = ga.genetic_approx(img, 48, 48, None, polish_steps=20, **kw)
    print("GA best", f0, "with polish", f1)
    assert f1 <= f0 and best.shape == (12, 9)
