"""The Adam refiner on the image loss (ggs_refine_create_loss, DeviceRefine(loss=)) on an
MI355X:

* B = 3 against K = 2 images with group 1 wants three images and is refused;
* B = 4, K = 2, group 2, N = 24 at 33 x 47 (height x width), 5 steps: the session's genomes,
  loss values, best and last gradient are bit for bit those of the host loop
  ``api.loss_grad`` + ``ggs.refine.adam_step``, and best_fits never exceeds the initial loss;
* a ``ggs_refine_create`` session run beside it keeps the bits of ``api.fitness_grad`` +
  ``adam_step`` (what tests/test_gpu_refine.py holds it to).
"""
from __future__ import annotations

import numpy as np
import pytest

import ggs
import ggs_oracle as oracle
from ggs import api, ga
from ggs.ga_device import DeviceRefine
from ggs.refine import DEFAULT_LR, AdamParams, adam_step, refine

pytestmark = pytest.mark.gpu
H, W, N = 33, 47, 24
MIN_S, MAX_S = 0.5, 0.5
LOSS = ggs.LossParams(0.8, 0.0, 0.2)
BG = (0.9, 0.8, 0.7)


def _problem():
    G = ga.clamp_genome(oracle.synthetic_population(4, N, H, W, seed=21), H, W, MIN_S, MAX_S)
    rng = np.random.default_rng(22)
    tg = np.stack([oracle.render(oracle.genome_to_renderer_batched(
        oracle.synthetic_population(1, 10, H, W, seed=30 + k)), H, W, k_sigma=3.0)[0] for k in range(2)])
    tg = np.clip(tg + rng.normal(0, 0.03, tg.shape), 0, 1).astype(np.float32)
    return np.ascontiguousarray(G), tg


def _session(G, tg, **kw):
    return DeviceRefine(tg, None, G, lr=DEFAULT_LR, min_scale_splats=MIN_S, max_scale_splats=MAX_S, **kw)


def test_three_candidates_against_two_images_are_refused():
    G, tg = _problem()
    with pytest.raises(ggs.GGSInputError, match="images wanted"):
        _session(G[:3], tg, loss=LOSS, group=1)


def test_five_steps_are_the_host_loop_bit_for_bit():
    G, tg = _problem()
    lo, hi = ga.scale_log_bounds(H, W, MIN_S, MAX_S)
    p = AdamParams(lr=DEFAULT_LR, log_lo=lo, log_hi=hi)
    kw = dict(k_sigma=3.0, background=BG, layout="axes", group=2)
    s = _session(G, tg, loss=LOSS, group=2, background=BG)
    # a plain fitness session beside it, stepped in turn
    t0 = tg[0]
    s0 = _session(G[:2], t0)
    x0, m0, v0 = G[:2].copy(), np.zeros_like(G[:2]), np.zeros_like(G[:2])

    r = s.read()
    first, _ = api.loss_grad(G, tg, H, W, LOSS, **kw)
    assert r["genomes"].tobytes() == G.tobytes() and r["fitness"].tobytes() == first.tobytes()
    assert r["best_fits"].tobytes() == first.tobytes() and not r["last_grad"].any()
    x, m, v = G.copy(), np.zeros_like(G), np.zeros_like(G)
    best, best_x = first.astype(np.float64), G.copy()
    for t in range(1, 6):
        s.run(1)
        r = s.read()
        loss, grad = api.loss_grad(x, tg, H, W, LOSS, **kw)
        assert r["last_grad"].tobytes() == grad.tobytes(), t
        x, m, v = adam_step(x, grad, m, v, t, p)
        assert r["genomes"].tobytes() == x.tobytes(), t
        now, _ = api.loss_grad(x, tg, H, W, LOSS, **kw)
        assert r["fitness"].tobytes() == now.tobytes(), t
        better = now.astype(np.float64) + 1e-10 < best
        best = np.where(better, now.astype(np.float64), best)
        best_x[better] = x[better]
        assert r["best_fits"].tobytes() == best.astype(np.float32).tobytes(), t
        assert r["best"].tobytes() == best_x.tobytes(), t
        assert (r["best_fits"] <= first).all()

        s0.run(1)
        r0 = s0.read()
        _, g0 = api.fitness_grad(x0, t0, H, W, 3.0)
        assert r0["last_grad"].tobytes() == g0.tobytes(), t
        x0, m0, v0 = adam_step(x0, g0, m0, v0, t, p)
        assert r0["genomes"].tobytes() == x0.tobytes(), t
        assert r0["fitness"].tobytes() == api.fitness(x0, t0, H, W, 3.0).tobytes(), t
    print("loss", first, "->", r["best_fits"])
    s.close()
    s0.close()


def test_refine_takes_the_loss_and_lowers_it():
    G, tg = _problem()
    first, _ = api.loss_grad(G, tg, H, W, LOSS, group=2)
    out = refine(G, tg, H, W, 20, min_scale_splats=MIN_S, max_scale_splats=MAX_S, loss=LOSS, group=2)
    print("loss", first, "->", out["best_fits"])
    assert (out["best_fits"] < first).all()
    again, _ = api.loss_grad(out["best"], tg, H, W, LOSS, group=2)
    assert again.tobytes() == out["best_fits"].tobytes()
    # one target for all candidates
    one = refine(G[:2], tg[0], H, W, 3, min_scale_splats=MIN_S, max_scale_splats=MAX_S, loss=LOSS)
    solo = refine(G[1:2], tg[0], H, W, 3, min_scale_splats=MIN_S, max_scale_splats=MAX_S, loss=LOSS)
    for k in ("genomes", "fitness", "best", "best_fits", "last_grad"):
        assert one[k][1].tobytes() == solo[k][0].tobytes(), k
