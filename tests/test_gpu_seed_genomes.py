"""Greedy coarse-to-fine seeding on an MI355X: ``ggs.seed_genomes`` (ggs_seed_genomes: every
round's render, placement and row writes on one stream) against the host loop
``ggs.seed.seed_genomes_host`` — the device's render, then the numpy statement, then the next
round, the pattern of the refine tests — bytewise; rows a round cannot place stay empty; a
genome of empty rows renders exactly the background; and the quality condition, whose inputs
tests/test_seed_host.py checks with the oracle first: a seeded genome scores below the empty
canvas and below the best of a random population."""
from __future__ import annotations

import numpy as np
import pytest

import _seed_cases as cases
import ggs
from ggs import seed as S
from ggs.ga import new_population, scale_log_bounds

pytestmark = pytest.mark.gpu
BG = (0.875, 0.75, 0.625)


def _host_loop(tgt, N, rounds, H, W, *, weights, k_sigma, bg):
    lo, _ = scale_log_bounds(H, W, 3.0, 0.1)
    render = lambda x: ggs.render(x, H, W, k_sigma=k_sigma, background=bg, layout="axes")  # noqa: E731
    return S.seed_genomes_host(tgt, N, rounds, render, weights=weights, log_lo=float(lo), background=bg)


def test_three_rounds_are_the_host_loop_bytewise():
    K, N, H, W = 2, 24, 33, 47
    tgt = cases.noisy_image(K, H, W, 11)
    tgt[:, 4:20, 6:30] = tgt[:, 4:5, 6:7]                      # a flat patch in the noise
    w = cases.weights(K, H, W, 12)
    f = lambda v: float(np.float32(np.log(v)))  # noqa: E731
    rounds = [S.SeedRound(16, 6, f(4.5), 220.0), S.SeedRound(8, 8, f(3.5), 200.0), S.SeedRound(4, 10, f(3.0), 160.0)]
    ref, rplaced = _host_loop(tgt, N, rounds, H, W, weights=w, k_sigma=3.0, bg=BG)
    assert rplaced.tolist() == [[6, 6], [8, 8], [10, 10]]       # every round places all its rows
    got, placed = ggs.seed_genomes(tgt, N, rounds, weights=w, k_sigma=3.0, background=BG)
    assert placed.tobytes() == rplaced.tobytes()
    assert got.tobytes() == ref.tobytes()
    # later rounds see the earlier ones: the two images' genomes differ and no row is left empty
    assert got[0].tobytes() != got[1].tobytes() and (got[..., 8] > 0).all()
    again, _ = ggs.seed_genomes(tgt, N, rounds, weights=w, k_sigma=3.0, background=BG)
    assert again.tobytes() == got.tobytes()
    solo, _ = ggs.seed_genomes(tgt[1], N, rounds, weights=w[1], k_sigma=3.0, background=BG)
    assert solo[0].tobytes() == got[1].tobytes()


def test_rows_a_round_cannot_place_stay_empty():
    K, N, H, W = 2, 12, 33, 47
    tgt = np.broadcast_to(np.asarray(BG, np.float32), (K, H, W, 3)).copy()
    tgt[0, 0:8, 0:8] = (0.0, 0.25, 0.5)                         # image 0: one wrong 16-cell; image 1: a perfect canvas
    f = lambda v: float(np.float32(np.log(v)))  # noqa: E731
    rounds = [S.SeedRound(16, 4, f(4.0), 255.0), S.SeedRound(4, 0, f(3.0), 255.0), S.SeedRound(8, 8, f(3.0), 255.0)]
    ref, rplaced = _host_loop(tgt, N, rounds, H, W, weights=None, k_sigma=3.0, bg=BG)
    assert rplaced[0].tolist() == [1, 0] and rplaced[1].tolist() == [0, 0] and rplaced[2, 1] == 0
    got, placed = ggs.seed_genomes(tgt, N, rounds, k_sigma=3.0, background=BG)
    assert placed.tobytes() == rplaced.tobytes() and got.tobytes() == ref.tobytes()
    lo, _ = scale_log_bounds(H, W, 3.0, 0.1)
    empty = S.empty_genome(N, lo)
    assert got[1].tobytes() == empty.tobytes()                  # nothing to fix: every row stays empty
    assert got[0, 1:4].tobytes() == empty[1:4].tobytes() and got[0, 0, 8] == 255.0
    k = int(placed[2, 0])
    assert got[0, 4 + k:].tobytes() == empty[4 + k:].tobytes()


@pytest.mark.parametrize("H,W", [(33, 47), (5, 1), (64, 64)])
def test_empty_rows_render_exactly_the_background(H, W):
    lo, _ = scale_log_bounds(H, W, 3.0, 0.1)
    img = ggs.render(S.empty_genome(7, lo, 2), H, W, background=BG, layout="axes")
    assert img.shape == (2, H, W, 3) and (img == np.asarray(BG, np.float32)).all()


def test_a_seeded_genome_beats_the_empty_canvas_and_a_random_population():
    H, W, N = cases.Q_H, cases.Q_W, cases.Q_N
    tgt, m = cases.rectangles_target(), cases.rectangles_mask()
    lo, _ = scale_log_bounds(H, W, 3.0, 0.1)
    g, placed = ggs.seed_genomes(tgt, N, cases.Q_ROUNDS, weights=m, k_sigma=cases.Q_K_SIGMA)
    fit = lambda pop: ggs.fitness(pop, tgt[0], H, W, cases.Q_K_SIGMA, weight_mask=m[0])  # noqa: E731
    seeded, empty = float(fit(g)[0]), float(fit(S.empty_genome(N, lo, 1))[0])
    rand = float(fit(new_population(cases.Q_P, N, H, W, 3.0, 0.1, np.random.default_rng(0))).min())
    print("seeded", seeded, "empty", empty, "best random of", cases.Q_P, rand, "placed", placed.tolist())
    assert placed.sum() == N
    assert seeded < empty and seeded < rand
