"""Island groups with a target per island (DeviceGAIslands with a 4-D target,
ggs_ga_islands_create_targets) on an MI355X.  Every comparison is exact: island k
runs the single-population kernels on its own slices against plan k, and a
genome's fitness does not depend on the batch it is evaluated in.

1. without migration island k IS DeviceGA(targets[k], masks[k], pops[k], seed=seeds[k]);
2. K copies of one target with migration: today's shared-target group, bit for bit
   (a re-scored migrant gets exactly the fitness it had);
3. distinct targets: a migration is ``ggs.ga.ring_migration(..., refit=...)`` with
   the immigrants' ``ggs.fitness`` against the destination's target and mask;
4. breeding after a migration continues as a fresh group created from the read
   state does (the re-ranked elites, the fused breed resuming);
5. GGS_GA_UNFUSED=1 and GGS_UNFUSED_FINALIZE=1 give the default run's bits;
6. ``ga.genetic_approx_many``.
"""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

import ggs
from ggs import ga
from ggs.ga_device import DeviceGA, DeviceGAIslands
from ggs.mask import compute_importance_mask, prepare_target

pytestmark = pytest.mark.gpu
CFG = dict(mut_sigma_max={"xy": 0.1, "alog": 0.5, "blog": 0.5, "theta": 0.3, "rgb": 25.0,
                          "alpha": 25.0},
           mut_sigma_min={"xy": 0.01, "alog": 0.05, "blog": 0.05, "theta": 0.025, "rgb": 2.0,
                          "alpha": 2.0},
           schedule="cosine")          # reference modules/config.py:22-43
MIN_S, MAX_S = 3.0, 0.1
_problems = {}


def _problem(H, W, K):
    """K images (distinct seeds, distinct sizes), their prepared targets [K, H, W, 3] and masks [K, H, W]."""
    if (H, W, K) not in _problems:
        images = [np.random.default_rng(H * 1000 + W + 31 * k).uniform(0, 255, (H + 9 + k, W + 5 + 2 * k, 3))
                  .astype(np.float32) for k in range(K)]
        t = np.stack([prepare_target(im, H, W) for im in images])
        m = np.stack([compute_importance_mask(x, H, W, smooth=3, strength=0.7) for x in t]).astype(np.float32)
        _problems[H, W, K] = (images, t, m)
    return _problems[H, W, K]


def _kw(tour_k, elite_k, cxpb=0.5, mutpb=0.2):
    return dict(tour_k=tour_k, elite_k=elite_k, cxpb=cxpb, mutpb=mutpb, min_scale_splats=MIN_S,
                max_scale_splats=MAX_S, **CFG)


def _pops(K, P, N, H, W, seeds):
    return np.stack([ga.new_population(P, N, H, W, MIN_S, MAX_S, np.random.default_rng(s)) for s in seeds])


def _assert_island_equals_session(grp, k, solo, what):
    np.testing.assert_array_equal(grp["population"][k], solo["population"], err_msg=f"{what}: island {k}")
    np.testing.assert_array_equal(grp["fitness"][k], solo["fitness"], err_msg=f"{what}: island {k}")
    np.testing.assert_array_equal(grp["best"][k], solo["best"], err_msg=f"{what}: island {k}")
    assert grp["best_fit"][k] == solo["best_fit"], (what, k)
    assert grp["curves"][k] == solo["curves"], (what, k)


def _assert_groups_equal(a, b, what, best=True):
    np.testing.assert_array_equal(a["population"], b["population"], err_msg=what)
    np.testing.assert_array_equal(a["fitness"], b["fitness"], err_msg=what)
    if best:
        np.testing.assert_array_equal(a["best"], b["best"], err_msg=what)
        np.testing.assert_array_equal(a["best_fit"], b["best_fit"], err_msg=what)
        assert a["curves"] == b["curves"], what


def _run_group(t, m, pops, seeds, every, mig, runs, total, **kw):
    """States after each (first, n) of `runs`."""
    g = DeviceGAIslands(t, m, pops, seeds, every, mig, **kw)
    try:
        out = []
        for first, n in runs:
            g.run(first, n, total)
            out.append(g.read())
        return out
    finally:
        g.close()


# ---- 1. no migration ---------------------------------------------------------------
SHAPES = [
    # H, W, K, P, N, elite, tour_k, G
    (40, 40, 3, 7, 33, 2, 3, 5),       # odd P, odd K, partial tile
    (128, 512, 2, 6, 16, 2, 2, 3),     # the smallest canvas with the finalize folded into the raster
    (40, 40, 2, 12, 700, 2, 2, 3),     # the saturation instances, 1024-thread breed workgroups
    (24, 24, 3, 8, 20, 8, 2, 3),       # elite == P: nothing evaluated
    (24, 24, 2, 6, 1, 0, 2, 3),        # N = 1, elite_k 0 -> 1
]


@pytest.mark.parametrize("H,W,K,P,N,elite,tour_k,G", SHAPES)
def test_islands_without_migration_are_sessions_on_their_own_target(H, W, K, P, N, elite, tour_k, G):
    _, t, m = _problem(H, W, K)
    seeds = [100 + 7 * k for k in range(K)]
    pops = _pops(K, P, N, H, W, seeds)
    kw = _kw(tour_k, elite)
    gmid, gend = _run_group(t, m, pops, seeds, 0, 0, [(1, 2), (3, G - 2)], G, **kw)
    assert len(gend["curves"][0]["best"]) == G + 1
    distinct = set()
    for k in range(K):
        solo = DeviceGA(t[k], m[k], pops[k], seed=seeds[k], **kw)
        try:
            solo.run(1, 2, G)
            smid = solo.read()
            solo.run(3, G - 2, G)
            send = solo.read()
        finally:
            solo.close()
        _assert_island_equals_session(gmid, k, smid, "after generation 2")
        _assert_island_equals_session(gend, k, send, f"after generation {G}")
        distinct.add(float(send["best_fit"]))
    assert len(distinct) == K          # the islands really were scored against different images


# ---- 2. K copies of one target -----------------------------------------------------
def test_copies_of_one_target_with_migration_are_the_shared_target_group():
    H = W = 40
    K, P, N, G = 3, 8, 20, 5
    _, t, m = _problem(H, W, 1)
    seeds = [11, 22, 33]
    pops = _pops(K, P, N, H, W, seeds)
    kw = _kw(2, 2)
    runs = [(1, 2), (3, 2), (5, 1)]                   # reads after the migrations at 2 and 4, and at the end
    shared = _run_group(t[0], m[0], pops, seeds, 2, 2, runs, G, **kw)
    copies = _run_group(np.repeat(t, K, axis=0), np.repeat(m, K, axis=0), pops, seeds, 2, 2, runs, G, **kw)
    (plain,) = _run_group(t[0], m[0], pops, seeds, 0, 0, [(1, G)], G, **kw)
    assert not np.array_equal(plain["population"], shared[-1]["population"])      # migrations happened
    for a, b, (first, n) in zip(copies, shared, runs):
        _assert_groups_equal(a, b, f"after generation {first + n - 1}")


# ---- 3. a migration between distinct targets ------------------------------------------
def _refit(t, m, H, W):
    return lambda k, genomes: ggs.fitness(genomes, t[k], H, W, 3.0, weight_mask=m[k])


MH = MW = 40
MK, MP, MN, ME = 3, 8, 33, 4
MSEEDS = [11, 22, 33]


@pytest.fixture(scope="module")
def migration_states():
    """A: no migration, generations 1..4.  B: migrate_every 4, m = 2, read after
    generations 4 and 5 (total 8 for both).  (Tied fitness values: the K = 2 test below.)"""
    _, t, m = _problem(MH, MW, MK)
    pops = _pops(MK, MP, MN, MH, MW, MSEEDS)
    kw = _kw(2, ME)
    (a4,) = _run_group(t, m, pops, MSEEDS, 0, 0, [(1, 4)], 8, **kw)
    b4, b5 = _run_group(t, m, pops, MSEEDS, 4, 2, [(1, 4), (5, 1)], 8, **kw)
    return t, m, kw, a4, b4, b5


def test_migration_rescoring_is_the_numpy_rule(migration_states):
    t, m, _, a4, b4, _ = migration_states
    want_p, want_f = ga.ring_migration(a4["population"], a4["fitness"], 2, refit=_refit(t, m, MH, MW))
    plain_p, plain_f = ga.ring_migration(a4["population"], a4["fitness"], 2)
    np.testing.assert_array_equal(want_p, plain_p)              # the same rows move ...
    assert not np.array_equal(want_f, plain_f)                  # ... with another fitness
    np.testing.assert_array_equal(b4["population"], want_p)
    np.testing.assert_array_equal(b4["fitness"], want_f)
    # best-so-far and curves are not touched by a migration
    np.testing.assert_array_equal(b4["best"], a4["best"])
    np.testing.assert_array_equal(b4["best_fit"], a4["best_fit"])
    assert b4["curves"] == a4["curves"]


def test_migration_half_the_population_two_islands_tie_among_the_replaced():
    """K = 2, m = P / 2, elite_k = P: nothing is ever replaced by offspring.  Rows 1
    and 5 of island 0 are copies of its worst row: they sit, tied, at the two worst
    ranks, where the tie rule decides which immigrant lands on which row."""
    H = W = 24
    K, P, N = 2, 8, 20
    _, t, m = _problem(H, W, K)
    seeds = [5, 6]
    pops = _pops(K, P, N, H, W, seeds)
    f0 = ggs.fitness(pops[0], t[0], H, W, 3.0, weight_mask=m[0])
    pops[0, 1] = pops[0, 5] = pops[0, int(np.argmax(f0))]
    kw = _kw(2, P)
    (a,) = _run_group(t, m, pops, seeds, 0, 0, [(1, 2)], 4, **kw)
    (b,) = _run_group(t, m, pops, seeds, 2, P // 2, [(1, 2)], 4, **kw)
    fa = a["fitness"][0]
    assert fa[P - 1] == fa[P - 2] == fa.max()
    want_p, want_f = ga.ring_migration(a["population"], a["fitness"], P // 2, refit=_refit(t, m, H, W))
    assert len(set(want_f[0][-2:].tolist())) == 2        # distinguishable immigrants on the tied rows
    np.testing.assert_array_equal(b["population"], want_p)
    np.testing.assert_array_equal(b["fitness"], want_f)
    np.testing.assert_array_equal(b["best"], a["best"])
    assert b["curves"] == a["curves"]


# ---- 4. after a migration ------------------------------------------------------------
def test_breeding_continues_after_a_rescored_migration(migration_states):
    """Generation 5 of B (bred from the migrated rows, their re-scored fitness and
    the re-ranked elites) against a fresh per-island-target group created from B's
    state after generation 4.  Best and curves start afresh there: not compared."""
    t, m, kw, _, b4, b5 = migration_states
    (fresh,) = _run_group(t, m, b4["population"], MSEEDS, 0, 0, [(5, 1)], 8, **kw)
    assert not np.array_equal(b5["population"], b4["population"])
    _assert_groups_equal(b5, fresh, "generation 5", best=False)
    # the fresh group evaluated the migrated rows itself: the installed fitness is the row's own
    (again,) = _run_group(t, m, b4["population"], MSEEDS, 0, 0, [(5, 0)], 8, **kw)
    np.testing.assert_array_equal(again["fitness"], b4["fitness"])


# ---- 5. the unfused switches ---------------------------------------------------------
UNFUSED = dict(H=128, W=512, K=2, P=6, N=16, elite=2, every=2, mig=1, G=5)   # a canvas whose finalize folds


def _unfused_case():
    c = UNFUSED
    _, t, m = _problem(c["H"], c["W"], c["K"])
    seeds = [3, 4]
    pops = _pops(c["K"], c["P"], c["N"], c["H"], c["W"], seeds)
    (end,) = _run_group(t, m, pops, seeds, c["every"], c["mig"], [(1, c["G"])], c["G"], **_kw(2, c["elite"]))
    return end


def _digest(st):
    return dict(population=st["population"], fitness=st["fitness"], best=st["best"], best_fit=st["best_fit"],
                curves=np.asarray([[c["best"], c["mean"], c["median"]] for c in st["curves"]]))


_UNFUSED_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import test_gpu_ga_multitarget as T
np.savez(sys.argv[3], **T._digest(T._unfused_case()))
"""


@pytest.mark.parametrize("switch", ["GGS_GA_UNFUSED", "GGS_UNFUSED_FINALIZE"])
def test_unfused_switches_give_the_same_bits(switch, tmp_path):
    """The switches are read once per process: a fresh child each."""
    pkg = os.path.dirname(os.path.dirname(ggs.__file__))
    path = str(tmp_path / "unfused.npz")
    subprocess.run([sys.executable, "-c", _UNFUSED_SCRIPT, pkg, os.path.dirname(__file__), path], check=True,
                   timeout=300, env=dict(os.environ, **{switch: "1"}))
    want = _digest(_unfused_case())
    un = np.load(path)
    for key, v in want.items():
        np.testing.assert_array_equal(un[key], v, err_msg=key)


# ---- 6. the public interface ---------------------------------------------------------
def test_genetic_approx_many_is_genetic_approx_per_image():
    H = W = 40
    K, seed = 3, 2**64 - 2            # seed + k wraps: (seed + k) mod 2^64
    images, _, _ = _problem(H, W, K)
    kw = dict(pop_size=8, n_splats=24, generations=4, tour_k=3, elite_k=2, cxpb=0.3, mutpb=0.1,
              min_scale_splats=MIN_S, max_scale_splats=MAX_S, k_sigma=3.0, mask_strength=0.7,
              boost_only=False, progress=False, **CFG)
    many = ga.genetic_approx_many(images, H, W, "cuda", seed=seed, return_state=True, **kw)
    plain = ga.genetic_approx_many(images, H, W, "cuda", seed=seed, **kw)
    assert len(many) == len(plain) == K
    for k in range(K):
        b, f, s = ga.genetic_approx(images[k], H, W, "cuda", seed=(seed + k) % 2**64, backend="device",
                                    return_state=True, **kw)
        np.testing.assert_array_equal(many[k][0], b)
        assert many[k][1] == f
        np.testing.assert_array_equal(many[k][2]["population"], s["population"])
        np.testing.assert_array_equal(many[k][2]["fitness"], s["fitness"])
        assert many[k][2]["curves"] == s["curves"]
        np.testing.assert_array_equal(plain[k][0], b)
        assert plain[k][1] == f and len(plain[k]) == 2
