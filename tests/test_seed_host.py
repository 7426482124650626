"""The numpy statement of residual-driven placement (ggs/seed.py) on the
CPU: the summation order against sums written out by hand, partial cells, one-pixel-wide
canvases, exact ties, the err_min rule, a perfect render, the default schedule, the
population builder, and the quality condition of the GPU test with the oracle's render."""
from __future__ import annotations

import numpy as np
import pytest

import ggs
import ggs_oracle as O
from ggs import seed as S
from ggs.ga import new_population, scale_log_bounds

import _seed_cases as cases

f32 = np.float32


def test_tree_sum_is_the_balanced_tree_not_the_running_sum():
    v = np.array([1e8, 1.0, -1e8, 1.0, 3.0, 1e-3, 5.0, 7.0], f32)
    hand = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]))
    assert S.tree_sum(v) == hand
    run = f32(0.0)
    for a in v:
        run = f32(run + a)
    assert run != hand                       # the order matters for these values
    # the xor-butterfly: lane l adds lane l ^ s for s = 1, 2, 4 and every lane ends on the tree's root
    w = v.copy()
    for s in (1, 2, 4):
        w = (w + w[np.arange(8) ^ s]).astype(f32)
    assert (w == hand).all()


def test_a_cell_sums_columns_top_down_then_the_tree():
    rng = np.random.default_rng(3)
    tgt = (rng.uniform(0, 1, (1, 4, 4, 3)) * np.array([1e4, 1.0, 1e-4])).astype(f32)
    img = np.zeros((1, 4, 4, 3), f32)
    w = rng.uniform(0.5, 1, (1, 4, 4)).astype(f32)
    d = img - tgt
    e = w * ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    assert e.dtype == f32
    cols = []
    for x in range(4):
        s = f32(0.0)
        for y in range(4):
            s = f32(s + e[0, y, x])
        cols.append(s)
    hand = f32(f32(cols[0] + cols[1]) + f32(cols[2] + cols[3]))
    cg = S.cell_grid(img, tgt, 4, weights=w)
    assert cg["err"].shape == (1, 1) and cg["err"][0, 0] == hand and cg["count"].tolist() == [16]
    tc = [f32(0.0)] * 4
    for x in range(4):
        for y in range(4):
            tc[x] = f32(tc[x] + tgt[0, y, x, 0])
    assert cg["sums"][0, 0, 0] == f32(f32(tc[0] + tc[1]) + f32(tc[2] + tc[3]))
    y, x = np.unravel_index(np.argmax(e[0]), (4, 4))
    assert cg["peak"][0, 0].tolist() == [y, x]


def test_partial_cells_count_only_the_image():
    H, W, c = 5, 7, 4
    tgt = np.full((1, H, W, 3), 0.5, f32)
    img = np.zeros((1, H, W, 3), f32)
    cg = S.cell_grid(img, tgt, c)
    assert (cg["Gy"], cg["Gx"]) == (2, 2) and cg["count"].tolist() == [16, 12, 4, 3]
    # every pixel's e is 0.75, sums of it are exact: err = 0.75 count, colour sums 0.5 count
    assert cg["err"][0].tolist() == [12.0, 9.0, 3.0, 2.25]
    assert cg["sums"][0, :, 1].tolist() == [8.0, 6.0, 2.0, 1.5]
    assert cg["peak"][0].tolist() == [[0, 0], [0, 4], [4, 0], [4, 4]]      # all tie: the first in (y, x)
    x, sites, n, _ = S.place_sites(np.zeros((1, 4, 9), f32), img, tgt, S.SeedParams(c, 4, 0, 0.0, 1.5, 99.0))
    assert n.tolist() == [4] and sites[0].tolist() == [0, 1, 2, 3]
    assert x[0, 1].tolist() == [f32(4) / f32(6), 0.0, 1.5, 1.5, 0.0, 127.5, 127.5, 127.5, 99.0]
    assert x[0, 3, :2].tolist() == [f32(4) / f32(6), 1.0]


@pytest.mark.parametrize("H,W", [(5, 1), (1, 5), (1, 1)])
def test_one_pixel_wide_canvases_divide_by_one(H, W):
    tgt = np.zeros((1, H, W, 3), f32)
    tgt[0, H - 1, W - 1] = 1.0
    x, sites, n, err = S.place_sites(np.zeros((1, 3, 9), f32), None, tgt[0], S.SeedParams(4, 3, 0, 0.0, 0.0, 10.0),
                                     background=(0.0, 0.0, 0.0))
    G = -(-H // 4) * -(-W // 4)
    assert err.shape == (1, G) and n.tolist() == [1] and sites[0].tolist() == [G - 1, -1, -1]
    px, py = W - 1, H - 1
    assert x[0, 0, 0] == f32(px) / f32(max(W - 1, 1)) and x[0, 0, 1] == f32(py) / f32(max(H - 1, 1))
    assert not x[0, 1:].any()


def test_exact_ties_go_to_the_lower_cell_and_the_smaller_pixel():
    tgt = np.zeros((1, 8, 16, 3), f32)
    tgt[0, :, :, 0] = 0.5                         # eight flat 4 x 4 cells, all with err 4.0
    tgt[0, 5, 9] = (0.5, 0.5, 0.0)                # cell 6 is larger, its peak is that pixel
    img = np.zeros((1, 8, 16, 3), f32)
    cg = S.cell_grid(img, tgt, 4)
    assert cg["err"][0].tolist() == [4.0] * 6 + [4.25, 4.0]
    sites, n = S.rank_sites(cg["err"], 0.0, 5)
    assert n.tolist() == [5] and sites[0].tolist() == [6, 0, 1, 2, 3]
    assert cg["peak"][0, 6].tolist() == [5, 9] and cg["peak"][0, 5].tolist() == [4, 4]
    # two equal maxima in one cell: the smaller y wins, then the smaller x
    tgt[0, 6, 8] = (0.5, 0.5, 0.0)
    tgt[0, 5, 11] = (0.5, 0.5, 0.0)
    assert S.cell_grid(img, tgt, 4)["peak"][0, 6].tolist() == [5, 9]


def test_err_min_excludes_cells_at_or_below_it():
    err = np.array([[4.0, 2.0, 2.5, 0.0, np.nan, 2.0]], f32)
    sites, n = S.rank_sites(err, 2.0, 6)
    assert n.tolist() == [2] and sites[0].tolist() == [0, 2, -1, -1, -1, -1]
    sites, n = S.rank_sites(err, 0.0, 2)
    assert n.tolist() == [2] and sites[0].tolist() == [0, 2]
    sites, n = S.rank_sites(err, 0.0, 6)
    assert n.tolist() == [4] and sites[0].tolist() == [0, 2, 1, 5, -1, -1]


def test_a_perfect_render_places_nothing_and_leaves_every_byte():
    tgt = cases.flat_targets(2, 33, 47, 1)
    x = cases.genomes(2, 12, 2)
    out, sites, n, err = S.place_sites(x, tgt.copy(), tgt, S.SeedParams(8, 12, 0, 0.0, 1.0, 200.0))
    assert n.tolist() == [0, 0] and (sites == -1).all() and not err.any()
    assert out.tobytes() == x.tobytes()


def test_the_group_rule_picks_the_target():
    tgt = cases.flat_targets(2, 16, 16, 4)
    img = cases.noisy_image(4, 16, 16, 5)
    both = S.cell_grid(img, tgt, 8, group=2)["err"]
    for b in range(4):
        assert both[b].tobytes() == S.cell_grid(img[b], tgt[b // 2], 8)["err"][0].tobytes()
    with pytest.raises(ggs.GGSInputError, match="group"):
        S.cell_grid(img, tgt, 8, group=3)


@pytest.mark.parametrize("N,H,W", [(512, 512, 512), (24, 33, 47), (7, 5, 1), (1, 64, 64), (100, 16, 300), (5000, 64, 64)])
def test_schedule_counts_sum_to_n_coarse_first(N, H, W):
    rs = S.seed_schedule(N, H, W)
    assert sum(r.count for r in rs) == N and all(r.count >= 0 for r in rs)
    cells = [r.cell for r in rs]
    assert cells == sorted(cells, reverse=True) and set(cells) <= set(S.CELLS) and 1 <= len(rs) <= 4
    lo, hi = scale_log_bounds(H, W, 3.0, 0.1)
    for r in rs[:-1]:
        assert r.count <= -(-H // r.cell) * -(-W // r.cell)
    assert all(min(lo, hi) <= r.log_sigma <= max(lo, hi) and 0 <= r.alpha <= 255 for r in rs)
    S.seed_rounds_c(rs, N)


def test_empty_rows_and_the_oracle_render_of_them():
    lo, _ = scale_log_bounds(20, 28, 3.0, 0.1)
    e = S.empty_genome(5, lo, 2)
    assert e.shape == (2, 5, 9) and e[1, 3].tolist() == [0.5, 0.5, lo, lo, 0, 0, 0, 0, 0]
    bg = (0.25, 0.5, 0.75)
    img = O.render(O.genome_to_renderer_batched(e), 20, 28, background=bg)
    assert (img == np.asarray(bg, f32)).all()


def test_seeded_population_keeps_the_genome_and_a_subset_of_its_rows():
    g = cases.genomes(1, 40, 7)[0]
    pop = S.seeded_population(6, g, 32, 32, np.random.default_rng(5), keep=0.5)
    assert pop.shape == (6, 40, 9) and pop.dtype == f32 and pop[0].tobytes() == g.tobytes()
    again = S.seeded_population(6, g, 32, 32, np.random.default_rng(5), keep=0.5)
    assert again.tobytes() == pop.tobytes()
    fresh = new_population(5, 40, 32, 32, 3.0, 0.1, np.random.default_rng(5))
    kept = (pop[1:] == g[None]).all(axis=2)
    assert 0.3 < kept.mean() < 0.7
    assert (pop[1:][~kept] == fresh[~kept]).all()        # the rest are new_population's rows of the same rng
    assert (S.seeded_population(3, g, 32, 32, np.random.default_rng(1), keep=1.0) == g[None]).all()
    with pytest.raises(ggs.GGSInputError):
        S.seeded_population(3, g, 32, 32, np.random.default_rng(1), keep=1.5)


def test_host_seeding_fills_rows_in_order_and_leaves_unplaced_rows_empty():
    H, W, N = 16, 16, 10
    tgt = np.ones((1, H, W, 3), f32)
    tgt[0, 0:8, 0:8] = 0.0                               # one 8 x 8 cell is wrong, the rest is the background
    lo, _ = scale_log_bounds(H, W, 3.0, 0.1)
    render = lambda x: O.render(O.genome_to_renderer_batched(x), H, W)  # noqa: E731
    rounds = [S.SeedRound(8, 4, 0.5, 255.0), S.SeedRound(4, 6, 0.25, 128.0)]
    g, placed = S.seed_genomes_host(tgt, N, rounds, render, log_lo=float(lo))
    assert placed[0].tolist() == [1] and 1 <= placed[1, 0] <= 6
    empty = S.empty_genome(N, lo)
    assert g[0, 0, 8] == 255.0 and g[0, 0, 2] == f32(0.5)
    assert g[0, 1:4].tobytes() == empty[1:4].tobytes()   # round 0 could place one of its four rows
    k = int(placed[1, 0])
    assert (g[0, 4:4 + k, 8] == 128.0).all() and g[0, 4 + k:].tobytes() == empty[4 + k:].tobytes()


def test_quality_condition_holds_for_the_statement_with_the_oracle_render():
    """The inequality tests/test_gpu_seed_genomes.py asserts on the device, here with the
    oracle's render and fitness: the seeded genome is below the empty canvas and below the
    best of a seeded-RNG new_population of the same P, with a visible margin."""
    H, W, N = cases.Q_H, cases.Q_W, cases.Q_N
    tgt, m = cases.rectangles_target(), cases.rectangles_mask()
    lo, _ = scale_log_bounds(H, W, 3.0, 0.1)
    render = lambda x: O.render(O.genome_to_renderer_batched(x), H, W, k_sigma=cases.Q_K_SIGMA)  # noqa: E731
    g, placed = S.seed_genomes_host(tgt, N, cases.Q_ROUNDS, render, weights=m, log_lo=float(lo))
    fit = lambda pop: O.fitness_many(list(pop), tgt[0], H, W, cases.Q_K_SIGMA, weight_mask=m[0])  # noqa: E731
    seeded, empty = float(fit(g)[0]), float(fit(S.empty_genome(N, lo, 1))[0])
    rand = float(fit(new_population(cases.Q_P, N, H, W, 3.0, 0.1, np.random.default_rng(0))).min())
    print("seeded", seeded, "empty", empty, "best random", rand, "placed", placed.tolist())
    assert placed.sum() == N
    assert seeded < 0.75 * empty and seeded < 0.75 * rand
