"""ggs/de.py, the numpy statement of the device DE, on the CPU:

* the index de-collision is exhaustive-checked for P = 4 .. 9;
* no word of a generation's Philox layout (tests/_philox_de.py) feeds two draws,
  and the vectorised draws are the layout walked word by word;
* crossover limits, bit-identical inheritance (wrapped angles included), the
  selection's NaN and tie rules;
* the host loop on a sum of squares is monotone in every statistic.
"""
from __future__ import annotations

import itertools
from collections import Counter

import numpy as np
import pytest

import _philox as X
import _philox_de as XD
from ggs import de
from ggs.ga import wrap_angle

LO, HI = np.float32(-1.0), np.float32(3.0)
KW = dict(f_lo=0.5, f_hi=0.9, cr=0.3, log_lo=LO, log_hi=HI)


@pytest.mark.parametrize("P", range(4, 10))
def test_decollide_is_distinct_and_uniform(P):
    for i in range(P):
        hits = Counter()
        for raw in itertools.product(range(P - 1), range(P - 2), range(P - 3)):
            r = de.de_decollide(i, raw)
            assert len({i, *r}) == 4 and all(0 <= v < P for v in r), (i, raw, r)
            hits[r] += 1
        # a bijection: every ordered triple of distinct rows != i exactly once
        want = {t for t in itertools.permutations([v for v in range(P) if v != i], 3)}
        assert set(hits) == want and set(hits.values()) == {1}


@pytest.mark.parametrize("per_splat", [False, True])
@pytest.mark.parametrize("P,N", [(4, 1), (5, 7)])
def test_no_word_feeds_two_draws(P, N, per_splat):
    entries = list(XD.layout(P, N, per_splat))
    words = [w for _, w in entries]
    assert len(set(words)) == len(words)
    assert len({d for d, _ in entries}) == len(entries)
    assert all(w[0] == XD.S_DE == 9 and 0 <= w[3] < 4 for w in words)
    assert XD.S_DE not in (X.S_MASK, X.S_NORM_A, X.S_NORM_B, X.S_NORM_C, X.S_IND, X.S_TOUR, X.S_CX, X.S_ACCEPT)
    n_cr = P * N * (1 if per_splat else 9)
    assert len(entries) == 5 * P + n_cr


@pytest.mark.parametrize("per_splat", [False, True])
def test_vectorised_draws_follow_the_layout(per_splat):
    seed, gen, P, N = 2**63 + 12345, 1000, 6, 5
    d = XD.draws(seed, gen, P, N, per_splat)
    assert d["r"].dtype == np.int32 and d["r"].shape == (P, 3) and d["cr_u"].shape == (P, N, 9)
    raw = {}
    for draw, (st, who, what, word) in XD.layout(P, N, per_splat):
        x = int(X.block(seed, gen, who, what, st)[word])
        if draw[0] in ("r1", "r2", "r3"):
            raw[draw] = x
        elif draw[0] == "jrand":
            assert d["jrand"][draw[1]] == x % (N if per_splat else 9 * N)
        elif draw[0] == "f_u":
            assert d["f_u"][draw[1]] == X.u01(x)
        else:
            assert d["cr_u"][draw[1:]] == X.u01(x), draw
    for i in range(P):
        want = de.de_decollide(i, [raw[(f"r{k + 1}", i)] % (P - 1 - k) for k in range(3)])
        assert tuple(d["r"][i]) == want
    assert 0.0 <= d["cr_u"].min() and d["cr_u"].max() < 1.0


def _state(P=6, N=5, seed=0):
    rng = np.random.default_rng(seed)
    pop = np.concatenate([rng.random((P, N, 2)), rng.uniform(LO, HI, (P, N, 2)), rng.uniform(-np.pi, np.pi, (P, N, 1)),
                          rng.uniform(0, 255, (P, N, 4))], axis=-1).astype(np.float32)
    return pop, rng.random(P).astype(np.float32)


@pytest.mark.parametrize("strategy", sorted(de.STRATEGIES))
def test_cr_zero_takes_one_gene_or_one_splat(strategy):
    pop, fits = _state()
    P, N, _ = pop.shape
    for cx in ("gene", "splat"):
        d = XD.draws(3, 1, P, N, cx == "splat")
        t = de.de_trials(pop, fits, d, strategy=strategy, crossover=cx, **dict(KW, cr=0.0))
        full = de.de_trials(pop, fits, d, strategy=strategy, crossover=cx, **dict(KW, cr=1.0))
        for i in range(P):
            j = int(d["jrand"][i])
            taken = np.zeros((N, 9), bool)
            if cx == "gene":
                taken[j // 9, j % 9] = True
            else:
                taken[j] = True
            np.testing.assert_array_equal(t[i][~taken].view(np.uint32), pop[i][~taken].view(np.uint32))
            np.testing.assert_array_equal(t[i][taken].view(np.uint32), full[i][taken].view(np.uint32))


def test_cr_one_and_zero_f_is_the_clamped_r1():
    pop, fits = _state()
    pop[..., 4] *= 3.0                               # angles outside [-pi, pi): the clamp wraps them
    pop[..., 0] += 0.5                               # x past 1: the clamp clips it
    P, N, _ = pop.shape
    d = XD.draws(5, 2, P, N, False)
    t = de.de_trials(pop, fits, d, strategy="rand1", crossover="gene", f_lo=0.0, f_hi=0.0, cr=1.0,
                     log_lo=LO, log_hi=HI)
    want = de._clamp_mutant(pop[d["r"][:, 0]], LO, HI)
    assert not np.array_equal(want, pop[d["r"][:, 0]])
    np.testing.assert_array_equal(t, want)


@pytest.mark.parametrize("cx", ["gene", "splat"])
def test_inherited_genes_are_the_parents_bits(cx):
    pop, fits = _state(P=8, N=40)
    # angles that wrap_angle moves: just inside the interval they shift by an ulp or so,
    # outside it by multiples of 2 pi
    th = np.linspace(-3.1, 3.1, pop[..., 4].size).astype(np.float32).reshape(pop[..., 4].shape)
    th[:, ::5] += np.float32(7.0)
    moved = wrap_angle(th) != th
    assert moved.mean() > 0.3, moved.mean()
    pop[..., 4] = th
    P, N, _ = pop.shape
    d = XD.draws(11, 4, P, N, cx == "splat")
    for strategy in de.STRATEGIES:
        t = de.de_trials(pop, fits, d, strategy=strategy, crossover=cx, **KW)
        if cx == "gene":
            take = ((d["cr_u"] < np.float32(KW["cr"])).reshape(P, -1) |
                    (np.arange(9 * N)[None] == d["jrand"][:, None])).reshape(P, N, 9)
        else:
            take = np.repeat(((d["cr_u"][:, :, 0] < np.float32(KW["cr"])) |
                              (np.arange(N)[None] == d["jrand"][:, None]))[:, :, None], 9, axis=2)
        kept = ~take
        assert (kept[..., 4] & moved).sum() > 20          # inherited angles that a re-wrap would change
        np.testing.assert_array_equal(t[kept].view(np.uint32), pop[kept].view(np.uint32))
        assert (t[take] != pop[take]).mean() > 0.5


def test_select_keeps_the_parent_on_nan_and_takes_the_trial_on_a_tie():
    pop = np.zeros((4, 2, 9), np.float32)
    trials = np.ones((4, 2, 9), np.float32)
    fits = np.array([1.0, 1.0, 1.0, np.nan], np.float32)
    tf = np.array([np.nan, 1.0, 2.0, 0.5], np.float32)
    p, f = de.de_select(pop, fits, trials, tf)
    assert [float(v[0, 0]) for v in p] == [0.0, 1.0, 0.0, 0.0]
    np.testing.assert_array_equal(f, fits)
    assert p.dtype == f.dtype == np.float32


def test_stats_are_the_gas():
    f = np.array([3.0, 1.0, 2.0, 1.0], np.float32)
    assert de.de_stats(f) == (1, 7.0 / 4.0, 1.5)
    assert de.de_stats(f[:3]) == (1, 2.0, 2.0)
    assert de.best_row(np.array([np.nan, 1.0], np.float32)) == 0


@pytest.mark.parametrize("strategy", sorted(de.STRATEGIES))
@pytest.mark.parametrize("cx", ["gene", "splat"])
def test_host_loop_is_monotone_on_a_sum_of_squares(strategy, cx):
    P, N, G = 12, 6, 20
    pop, _ = _state(P, N, seed=1)
    goal = _state(1, N, seed=2)[0][0]

    def evaluate(g):
        return ((g.astype(np.float64) - goal) ** 2).sum(axis=(1, 2)).astype(np.float32)

    src = XD.PhiloxDeDraws(9, cx)
    state = None
    fits_by_gen = []
    for g in range(0, G + 1):                        # generation by generation, to see every fitness vector
        state = de.run_host_de(pop, 0 if g == 0 else 1, src, evaluate, strategy=strategy, crossover=cx,
                               first_gen=g, state=state, **KW)
        fits_by_gen.append(state["fitness"].copy())
    whole = de.run_host_de(pop, G, src, evaluate, strategy=strategy, crossover=cx, **KW)
    np.testing.assert_array_equal(whole["population"], state["population"])
    assert whole["curves"] == state["curves"] and whole["best_fit"] == state["best_fit"]
    c = whole["curves"]
    assert len(c["best"]) == len(c["mean"]) == len(c["median"]) == G + 1
    for a, b in zip(fits_by_gen, fits_by_gen[1:]):
        assert (b <= a).all()
    for k in ("best", "mean", "median"):
        assert all(y <= x for x, y in zip(c[k], c[k][1:])), k
    assert c["best"][-1] < c["best"][0]
    assert whole["best_fit"] == float(evaluate(whole["best"][None])[0]) == c["best"][-1]


def test_differential_evolution_host_backend_with_an_evaluate_hook():
    H = W = 16
    P, N, G = 6, 3, 4
    target = np.random.default_rng(0).uniform(0, 255, (H, W, 3)).astype(np.float32)
    calls = []

    def evaluate(g):
        calls.append(len(g))
        return (g.astype(np.float64) ** 2).sum(axis=(1, 2)).astype(np.float32)

    kw = dict(min_scale_splats=0.5, max_scale_splats=0.5, k_sigma=3.0, mask_strength=0.7, boost_only=False,
              progress=False, evaluate=evaluate, seed=3)
    b, f, st = de.differential_evolution(target, H, W, "cpu", P, N, G, return_state=True, **kw)
    assert calls == [P] * (G + 1)
    assert b.shape == (N, 9) and st["population"].shape == (P, N, 9) and len(st["curves"]["best"]) == G + 1
    b2, f2 = de.differential_evolution(target, H, W, "cpu", P, N, G, **kw)
    np.testing.assert_array_equal(b, b2)
    assert f == f2
    with pytest.raises(ValueError):
        de.differential_evolution(target, H, W, "cpu", 3, N, G, **kw)
    with pytest.raises(ValueError):
        de.differential_evolution(target, H, W, "cpu", P, N, G, strategy="rand2", **kw)
