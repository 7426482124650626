"""The in-kernel Philox draws of the device GA / SA (csrc/ggs_ga.hip) on an MI355X,
through the stage export ``ggs_ga_philox_draws`` (``ga_device.philox_draws``).

* the exported draws are those of the independent restatement tests/_philox.py:
  integer fields and uniforms bit for bit, normals within ``NORMAL_BAR`` of the
  float64 Box-Muller of the same words;
* the normals are standard normal and the index draws uniform at the 4-sigma level;
* closure: a Philox run IS the explicit-draw run on the exported draws, bit for
  bit — ``DeviceGA(seed).run`` against ``step(draws=philox_draws(...))`` on every
  variation instantiation, and (N <= 64) against the numpy GA of ggs/ga.py, which
  is replay-verified against the reference; ``DeviceSA.propose`` likewise.  The
  export kernel restates a few inline expressions of the variation kernels (the
  crossover decision and mask uniform, the tournament index, swap_i, swap_u):
  the closure is what proves the restatement is what the kernels do.
"""
from __future__ import annotations

import numpy as np
import pytest

import _philox as X
from ggs import ga
from ggs.ga_device import DeviceGA, DeviceSA, philox_draws
from test_gpu_ga import CFG, _problem
from test_philox_host import EDGE_U1_MIN, EDGE_U1_ONE

pytestmark = pytest.mark.gpu

INT_FIELDS = ("tour_idx", "perm", "cx", "k_color", "k_xy", "k_ab", "k_t", "swap_i", "swap_pick")
UNIFORMS = ("cx_u", "u_xy", "u_ab", "u_t", "u_rgb", "u_a", "swap_u")
NORMALS = ("n_xy", "n_ab", "n_t", "n_rgba")
# max |device normal - float64 Box-Muller of the same words|: see test_export_matches_restatement
NORMAL_MEASURED = 5.634e-7
NORMAL_BAR = 4 * NORMAL_MEASURED
SEEDS = (0, 42, 2**63 + 12345)
# Scale bounds of the closure tests.  clamp_genome keeps log scales in [log MIN_S, log(MAX_S max(H, W))];
# with the suite's usual (3.0, 0.1) that interval is empty below 30 pixels, every splat is clamped to one
# size and the size-ordered swap (swap_i, swap_u) never fires.  These keep it alive on 16 .. 40 pixel canvases.
MIN_S, MAX_S = 0.5, 0.5


def _normal_err(dev, ref):
    return max(float(np.abs(dev[k].astype(np.float64) - ref[k]).max()) for k in NORMALS)


@pytest.mark.parametrize("n_off,P,N,tour_k", [(5, 11, 37, 3), (2, 11, 1100, 3), (5, 11, 1, 3)])
@pytest.mark.parametrize("seed", SEEDS)
def test_export_matches_restatement(seed, n_off, P, N, tour_k):
    """Integer fields and uniforms bit-equal; normals within NORMAL_BAR of the
    float64 Box-Muller of the same words.

    Measured on an MI355X over these cases (3 seeds x gen 1, 1000 x first 0, 3 x
    the three shapes, 258,120 normals): max |device - float64| = 5.634e-7, bar 2.254e-6
    (the hardware log2 / sqrt / sin / cos chain of normal_pair).  The bar is 4x
    that: the figure is one sample, the factor leaves room for unseen words; the
    float32 spacing at |n| <= 5.8 is 4.8e-7 and every structural mistake (radians
    for revolutions, a wrong constant, words crossed between draws) is 0.1 - 1."""
    worst = 0.0
    for gen in (1, 1000):
        for first in (0, 3):
            dev = philox_draws(seed, gen, n_off, P, N, tour_k, 0.3, first=first)
            ref = X.draws(seed, gen, n_off, P, N, tour_k, 0.3, first=first)
            assert sorted(dev) == sorted(ref)
            for k in INT_FIELDS + UNIFORMS:
                assert dev[k].dtype == ref[k].dtype and dev[k].shape == ref[k].shape, k
                np.testing.assert_array_equal(dev[k], ref[k], err_msg=f"{k} gen {gen} first {first}")
            for k in NORMALS:
                assert dev[k].dtype == np.float32 and dev[k].shape == ref[k].shape, k
                assert np.isfinite(dev[k]).all(), k
            worst = max(worst, _normal_err(dev, ref))
    print(f"normal max |device - float64| = {worst:.3e} (seed {seed}, shape {(n_off, P, N, tour_k)})")
    assert worst <= NORMAL_BAR, worst


def test_normals_at_the_edge_words():
    """u1 = 1 (r = 0): both outputs exactly +-0.  u1 = 2^-24 (r = 5.768, the largest
    normal the generator can give): finite and within the bar of float64."""
    seed, gen, o, s, pi = EDGE_U1_ONE
    _, _, _, d1, d2 = X.NORMAL_PAIRS[pi]
    dev = philox_draws(seed, gen, o + 1, 2, s + 1, 1, 0.5)
    for f, c in (d1, d2):
        assert dev[f][o, s, c] == 0.0, (f, c, dev[f][o, s, c])
    seed, gen, o, s, pi = EDGE_U1_MIN
    _, _, _, d1, d2 = X.NORMAL_PAIRS[pi]
    dev = philox_draws(seed, gen, o + 1, 2, s + 1, 1, 0.5)
    ref = X.draws(seed, gen, o + 1, 2, s + 1, 1, 0.5)
    for dst in (d1, d2):
        if dst is not None:
            f, c = dst
            err = abs(float(dev[f][o, s, c]) - ref[f][o, s, c])
            print(f"u1 = 2^-24: {f}[{c}] device {dev[f][o, s, c]!r} float64 {ref[f][o, s, c]!r} err {err:.3e}")
            assert np.isfinite(dev[f][o, s, c]) and err <= NORMAL_BAR
    for k in NORMALS:
        assert np.isfinite(dev[k]).all() and _normal_err(dev, ref) <= NORMAL_BAR


# ---- distribution ---------------------------------------------------------------------------
STAT_SEED = 1          # chosen on the CPU: the float64 restatement meets every bound below
STAT_ARGS = (1, 64, 11, 512, 3)          # gen, n_off, P, N, tour_k: 294,912 normals, 229,376 mask uniforms
HIST_ARGS = (1, 4096, 11, 8, 4096)       # 45,056 tournament indices over 11 bins, 4,096 k_t over 8


def normal_stats(d):
    """(n, |mean|, |var - 1|, pairs, |corr| of the two outputs of the pairs that use both)."""
    allv = np.concatenate([np.asarray(d[k], np.float64).reshape(-1) for k in NORMALS])
    a = np.concatenate([d["n_xy"][..., 0], d["n_ab"][..., 0], d["n_t"][..., 0], d["n_rgba"][..., 1]],
                       axis=None).astype(np.float64)
    b = np.concatenate([d["n_xy"][..., 1], d["n_ab"][..., 1], d["n_rgba"][..., 0], d["n_rgba"][..., 2]],
                       axis=None).astype(np.float64)
    return allv.size, abs(allv.mean()), abs(allv.var() - 1.0), a.size, abs(np.corrcoef(a, b)[0, 1])


def normal_stats_ok(d):
    n, mean, var, m, corr = normal_stats(d)
    return mean <= 4 / np.sqrt(n) and var <= 4 * np.sqrt(2 / n) and corr <= 4 / np.sqrt(m)


def hist_ok(idx, bins):
    """Every bin of a uniform index within 4 sigma (binomial) of n / bins."""
    idx = np.asarray(idx).reshape(-1)
    n, p = idx.size, 1.0 / bins
    cnt = np.bincount(idx, minlength=bins)
    return len(cnt) == bins and bool((np.abs(cnt - n * p) <= 4 * np.sqrt(n * p * (1 - p))).all())


def test_normals_are_standard_normal():
    gen, n_off, P, N, tour_k = STAT_ARGS
    ref = X.draws(STAT_SEED, gen, n_off, P, N, tour_k, 0.5)
    assert normal_stats(ref)[0] == 294912 and sum(ref[k].size for k in UNIFORMS[1:6]) == 229376
    assert normal_stats_ok(ref), ("the seed no longer meets the condition", normal_stats(ref))
    dev = philox_draws(STAT_SEED, gen, n_off, P, N, tour_k, 0.5)
    print("device normals: n, |mean|, |var-1|, pairs, |corr| =", normal_stats(dev))
    assert normal_stats_ok(dev), normal_stats(dev)
    for k in UNIFORMS:
        np.testing.assert_array_equal(dev[k], ref[k], err_msg=k)
    u = np.concatenate([dev[k].reshape(-1) for k in UNIFORMS[1:6]]).astype(np.float64)
    assert abs(u.mean() - 0.5) <= 4 * np.sqrt(1 / 12 / u.size) and 0.0 <= u.min() and u.max() < 1.0


def test_index_draws_are_uniform():
    gen, n_off, P, N, tour_k = HIST_ARGS
    ref = X.draws(STAT_SEED, gen, n_off, P, N, tour_k, 0.5)
    assert hist_ok(ref["tour_idx"], P) and hist_ok(ref["k_t"], N), "the seed no longer meets the condition"
    assert hist_ok(ref["k_color"], 2 * N) and hist_ok(ref["swap_i"], N - 1)
    dev = philox_draws(STAT_SEED, gen, n_off, P, N, tour_k, 0.5)
    assert hist_ok(dev["tour_idx"], P), np.bincount(dev["tour_idx"].reshape(-1), minlength=P)
    assert hist_ok(dev["k_t"], N), np.bincount(dev["k_t"], minlength=N)
    assert hist_ok(dev["k_color"], 2 * N) and hist_ok(dev["k_xy"], 2 * N) and hist_ok(dev["k_ab"], 2 * N)
    assert hist_ok(dev["swap_i"], N - 1), np.bincount(dev["swap_i"], minlength=N - 1)


# ---- closure: GA -----------------------------------------------------------------------------
GA_SHAPES = [
    # H, W, P, N, G, tour_k, elite_k, cxpb, mutpb, boost
    (24, 24, 7, 33, 3, 3, 2, .5, .25, False),          # odd P (the last pair's slot wraps)
    (24, 24, 8, 300, 2, 2, 2, .5, .125, False),        # 512-thread path
    (24, 24, 6, 700, 2, 2, 2, .5, .125, False),        # 1024-thread path
    (24, 24, 6, 1100, 2, 2, 2, .5, .125, False),       # generic path
    (24, 24, 64, 1100, 2, 2, 4, .5, .125, False),      # generic path, P >= 64: 256 threads
    (16, 16, 600, 3, 2, 3, 25, .5, .125, False),       # P > 512: separate survivors
    (24, 24, 8, 2, 3, 2, 1, .25, 2.0 ** -10, False),   # rare mutation: fallbacks
    (24, 24, 6, 1, 3, 2, 0, .5, .5, False),            # N = 1: no swap; elite_k 0 -> 1
    (24, 24, 12, 30, 2, 40, 2, .5, .25, False),        # 2 tour_k > 64: the tournament loop
    (24, 24, 8, 20, 2, 2, 8, .5, .25, False),          # elite_k == P
    (24, 24, 7, 33, 3, 3, 2, .5, .25, True),           # boost_only
]


def _same_state(a, b, what):
    for k in ("population", "fitness", "best"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")
    assert a["best_fit"] == b["best_fit"], what
    for k in ("best", "mean", "median"):
        assert a["curves"][k] == b["curves"][k], (what, k)


@pytest.mark.parametrize("H,W,P,N,G,tour_k,elite_k,cxpb,mutpb,boost", GA_SHAPES)
def test_philox_run_is_the_explicit_run_on_the_exported_draws(H, W, P, N, G, tour_k, elite_k, cxpb, mutpb, boost):
    """cxpb and mutpb are powers of two: the host GA compares in double and the
    device in float32, and both must be the same predicate."""
    seed = 1000 + N
    target, t, m = _problem(H, W, N)
    init = ga.new_population(P, N, H, W, MIN_S, MAX_S, np.random.default_rng(N))
    kw = dict(tour_k=tour_k, elite_k=elite_k, cxpb=cxpb, mutpb=mutpb, min_scale_splats=MIN_S,
              max_scale_splats=MAX_S, boost_only=boost, **CFG)
    a, b = DeviceGA(t, m, init, seed=seed, **kw), DeviceGA(t, m, init, seed=seed + 1, **kw)
    try:
        a.run(1, G, G)                                  # Philox; fused breeds where P <= 512
        dicts = [philox_draws(seed, g, P, P, N, tour_k, cxpb) for g in range(1, G + 1)]
        for g in range(1, G + 1):
            b.step(g, G, dicts[g - 1])                  # explicit draws (b's own seed is not used)
        ra, rb = a.read(), b.read()
    finally:
        a.close()
        b.close()
    assert len(ra["curves"]["best"]) == G + 1
    if N >= 2:                                          # sizes differ, so the swap draws are consumed
        assert len(np.unique(ra["population"][..., 2:4])) > N
    _same_state(ra, rb, "device explicit")
    if N <= 64:                                         # the numpy GA on the same draws
        hb, hf, hs = ga.genetic_approx(target, H, W, "cuda", pop_size=P, n_splats=N, generations=G,
                                       tour_k=tour_k, elite_k=elite_k, cxpb=cxpb, mutpb=mutpb,
                                       min_scale_splats=MIN_S, max_scale_splats=MAX_S, k_sigma=3.0,
                                       mask_strength=0.7, boost_only=boost, init_population=init,
                                       progress=False, return_state=True, backend="host",
                                       draws=X.ExportedDraws(dicts), **CFG)
        _same_state(ra, dict(hs, best=hb, best_fit=hf), "numpy GA")


# ---- closure: SA proposer --------------------------------------------------------------------
def _sa_session(t, m, init, seed, mutpb, incremental):
    return DeviceSA(t, m, init, max_tries=4, mutpb=mutpb, min_scale_splats=MIN_S, max_scale_splats=MAX_S,
                    seed=seed, incremental=incremental, **CFG)


@pytest.mark.parametrize("H,W,N,mutpb,inc,calls", [
    (40, 40, 17, 0.25, False, [(0, 4), (3, 2)]),
    (32, 40, 1100, 0.25, False, [(0, 2)]),
    (96, 80, 64, 2.0 ** -9, True, [(0, 4), (1, 3)]),
])
def test_philox_propose_is_the_explicit_propose_on_the_exported_draws(H, W, N, mutpb, inc, calls):
    seed, it, total = 77 + N, 5, 20
    _, t, m = _problem(H, W, N)
    init = ga.new_population(1, N, H, W, MIN_S, MAX_S, np.random.default_rng(N))[0]
    a, b = _sa_session(t, m, init, seed, mutpb, inc), _sa_session(t, m, init, seed + 1, mutpb, inc)
    try:
        for first_try, n in calls:
            ea = a.propose(it, total, first_try, n)
            eb = b.propose(it, total, first_try, n,
                           draws=philox_draws(seed, it, n, n, N, 1, 0.0, first=first_try))
            np.testing.assert_array_equal(ea, eb)
            na, nb = a.read()[2], b.read()[2]
            assert na.shape == (n, N, 9)
            np.testing.assert_array_equal(na, nb)
            assert not np.array_equal(na[0], init) and len({x.tobytes() for x in na}) == n
            assert len(np.unique(na[..., 2:4])) > N     # sizes differ, so the swap draws are consumed
        # a try does not depend on how the tries are batched
        e4, n4 = a.propose(it, total, 0, 4), a.read()[2].copy()
        e01, n01 = a.propose(it, total, 0, 2), a.read()[2].copy()
        e23, n23 = a.propose(it, total, 2, 2), a.read()[2].copy()
        np.testing.assert_array_equal(e4, np.concatenate([e01, e23]))
        np.testing.assert_array_equal(n4, np.concatenate([n01, n23]))
    finally:
        a.close()
        b.close()
