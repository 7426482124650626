"""ggs.ga.polish_elites, the numpy statement of the island group's polish
(ggs_ga_islands_set_polish): the ranking, the strictly-lower install rule and the
argument errors, with a fake ``refine`` (no GPU)."""
from __future__ import annotations

import numpy as np
import pytest

from ggs import ga


def _group(K=2, P=6, N=3, seed=0):
    rng = np.random.default_rng(seed)
    return rng.random((K, P, N, 9), dtype=np.float32), rng.random((K, P), dtype=np.float32)


def test_the_ranked_rows_reach_refine_in_rank_order_ties_by_lower_row():
    pops, fits = _group()
    fits[0] = [0.5, 0.2, 0.2, 0.9, 0.1, 0.2]          # ranks: row 4, then 1, 2, 5 (ties by lower row)
    fits[1] = [0.3, 0.3, 0.3, 0.3, 0.3, 0.3]          # all tied: rows 0, 1, 2
    seen = {}

    def refine(k, g):
        seen[k] = g.copy()
        return g, np.full(len(g), np.inf, np.float32)

    ga.polish_elites(pops, fits, 3, refine)
    assert np.array_equal(seen[0], pops[0, [4, 1, 2]])
    assert np.array_equal(seen[1], pops[1, [0, 1, 2]])


def test_only_a_strictly_lower_fitness_installs_and_other_rows_keep_their_bits():
    pops, fits = _group(seed=1)
    fits[0] = [0.5, 0.2, 0.25, 0.9, 0.1, 0.3]
    fits[1] = [0.6, 0.5, 0.4, 0.3, 0.2, 0.1]
    marker = np.float32(7.0)

    def refine(k, g):
        # rank 0: lower; rank 1: equal (not installed); rank 2: higher (not installed)
        rows = np.argsort(fits[k], kind="stable")[:3]
        bf = fits[k, rows] + np.asarray([-0.05, 0.0, 0.05], np.float32)
        return np.full_like(g, marker), bf.astype(np.float32)

    p0, f0 = pops.copy(), fits.copy()
    new_p, new_f = ga.polish_elites(pops, fits, 3, refine)
    assert np.array_equal(pops, p0) and np.array_equal(fits, f0)      # new arrays
    for k, top in ((0, 4), (1, 5)):
        assert np.all(new_p[k, top] == marker) and new_f[k, top] == np.float32(fits[k, top] - np.float32(0.05))
        keep = [r for r in range(6) if r != top]
        assert new_p[k, keep].tobytes() == pops[k, keep].tobytes()
        assert new_f[k, keep].tobytes() == fits[k, keep].tobytes()


def test_a_nan_fitness_is_not_installed():
    pops, fits = _group(seed=2)
    new_p, new_f = ga.polish_elites(pops, fits, 2, lambda k, g: (g * 0, np.full(len(g), np.nan, np.float32)))
    assert new_p.tobytes() == pops.tobytes() and new_f.tobytes() == fits.tobytes()


@pytest.mark.parametrize("n_rows", [0, -1, 7])
def test_n_rows_outside_the_population_raises(n_rows):
    pops, fits = _group()
    with pytest.raises(ValueError):
        ga.polish_elites(pops, fits, n_rows, lambda k, g: (g, np.zeros(len(g), np.float32)))


def test_mismatched_shapes_raise():
    pops, fits = _group()
    with pytest.raises(ValueError):
        ga.polish_elites(pops, fits[:, :5], 1, lambda k, g: (g, np.zeros(len(g), np.float32)))


def test_a_group_of_one_and_every_row():
    pops, fits = _group(K=1)
    new_p, new_f = ga.polish_elites(pops, fits, 6, lambda k, g: (g + 1, np.full(len(g), -1.0, np.float32)))
    order = np.argsort(fits[0], kind="stable")
    assert np.all(new_f == -1.0)
    inv = np.empty(6, int)
    inv[order] = np.arange(6)
    assert np.array_equal(new_p[0], (pops[0, order] + 1)[inv])


@pytest.mark.parametrize("over,word", [(dict(memetic_rows=0), "memetic_rows"), (dict(memetic_every=-1), "memetic_every"),
                                       (dict(memetic_steps=-2), "memetic_steps"), (dict(backend="hots"), "backend"),
                                       (dict(backend="host"), "device session")])
def test_the_drivers_refuse_bad_memetic_arguments_before_any_work(over, word):
    zero = dict.fromkeys(("xy", "alog", "blog", "theta", "rgb", "alpha"), 0.0)
    kw = dict(pop_size=4, n_splats=2, generations=2, tour_k=2, elite_k=1, cxpb=0.5, mutpb=0.3, mut_sigma_max=zero,
              mut_sigma_min=zero, schedule="linear", min_scale_splats=0.5, max_scale_splats=0.5, k_sigma=3.0,
              mask_strength=0.5, boost_only=False, progress=False, memetic_every=2, memetic_steps=3)
    kw.update(over)
    with pytest.raises(ValueError, match=word):
        ga.genetic_approx(np.zeros((8, 8, 3), np.uint8), 8, 8, None, **kw)
