"""Memetic generations of the island group (ggs_ga_islands_set_polish,
DeviceGAIslands.set_polish) on an MI355X: 48 x 48, K = 3 islands of P = 8 rows,
N = 12 splats, tour_k 2, elite_k 2, two rows polished by three Adam steps, with a
shared target and with a target per island.  Every comparison is exact: a polish
is ``ggs.ga.polish_elites`` with a single-target ``DeviceRefine`` per island.

1. a polish is the numpy rule (and at least one row really is replaced);
2. a migration and a polish on the same generation: polish_elites(ring_migration(...));
3. breeding continues from the polished rows as a fresh group created from them does;
4. every = 0, n_steps = 0, NULL and an ``every`` never reached are a group that never
   called set_polish;
5. the best so far follows an improved top row, the curves already written stay;
6. GGS_GA_UNFUSED=1 gives the same bits; 7. a group of one; 8. the Python drivers.
"""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

import ggs
from ggs import ga
from ggs.ga_device import DeviceGAIslands, DeviceRefine
from ggs.mask import compute_importance_mask, prepare_target
from ggs.refine import DEFAULT_LR

pytestmark = pytest.mark.gpu
CFG = dict(mut_sigma_max={"xy": 0.1, "alog": 0.5, "blog": 0.5, "theta": 0.3, "rgb": 25.0, "alpha": 25.0},
           mut_sigma_min={"xy": 0.01, "alog": 0.05, "blog": 0.05, "theta": 0.025, "rgb": 2.0, "alpha": 2.0},
           schedule="cosine")
MIN_S, MAX_S = 3.0, 0.1
H = W = 48
K, P, N, ELITE, ROWS, STEPS = 3, 8, 12, 2, 2, 3
G, TOTAL = 3, 8                     # the polish (and the migration) after generation G
SEEDS = [11, 22, 33]
KW = dict(tour_k=2, elite_k=ELITE, cxpb=0.5, mutpb=0.2, min_scale_splats=MIN_S, max_scale_splats=MAX_S, **CFG)
_cache = {}


def _problem():
    if "p" not in _cache:
        images = [np.random.default_rng(4800 + 31 * k).uniform(0, 255, (H + 9 + k, W + 5 + 2 * k, 3))
                  .astype(np.float32) for k in range(K)]
        t = np.stack([prepare_target(im, H, W) for im in images])
        m = np.stack([compute_importance_mask(x, H, W, smooth=3, strength=0.7) for x in t]).astype(np.float32)
        pops = np.stack([ga.new_population(P, N, H, W, MIN_S, MAX_S, np.random.default_rng(s)) for s in SEEDS])
        _cache["p"] = (images, t, m, pops)
    return _cache["p"]


def _targets(kind):
    _, t, m, _ = _problem()
    return (t, m) if kind == "per_island" else (t[0], m[0])


def _group(kind, pops, every_mig=0, mig=0, polish=None, seeds=SEEDS):
    t, m = _targets(kind)
    if len(seeds) == 1 and kind == "per_island":
        t, m = t[:1], m[:1]
    g = DeviceGAIslands(t, m, pops, seeds, every_mig, mig, **KW)
    if polish is not None:
        polish(g)
    return g


def _run(kind, pops, runs, **kw):
    g = _group(kind, pops, **kw)
    try:
        out = []
        for first, n in runs:
            g.run(first, n, TOTAL)
            out.append(g.read())
        return out
    finally:
        g.close()


def _on(every=G, steps=STEPS, rows=ROWS):
    return lambda g: g.set_polish(every, steps, rows)


def _refine(kind):
    """polish_elites' ``refine``: a single-target refine session on island k's image."""
    _, t, m, _ = _problem()

    def refine(k, genomes):
        i = k if kind == "per_island" else 0
        s = DeviceRefine(t[i], m[i], genomes, lr=DEFAULT_LR, min_scale_splats=MIN_S, max_scale_splats=MAX_S)
        try:
            s.run(STEPS)
            r = s.read()
            return r["best"], r["best_fits"]
        finally:
            s.close()
    return refine


def _refit(k, genomes):
    _, t, m, _ = _problem()
    return ggs.fitness(genomes, t[k], H, W, 3.0, weight_mask=m[k])


@pytest.fixture(scope="module", params=["shared", "per_island"])
def states(request):
    """A: no polish, generations 1..G.  B: polish after generation G, read then and
    after two more generations."""
    kind = request.param
    pops = _problem()[3]
    (a,) = _run(kind, pops, [(1, G)])
    b, b2 = _run(kind, pops, [(1, G), (G + 1, 2)], polish=_on())
    return kind, a, b, b2


def _same(a, b, what, keys=("population", "fitness", "best", "best_fit")):
    for key in keys:
        assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), (what, key)


def test_a_polish_is_the_numpy_rule(states):
    kind, a, b, _ = states
    want_p, want_f = ga.polish_elites(a["population"], a["fitness"], ROWS, _refine(kind))
    replaced = int((want_f != a["fitness"]).sum())
    print(kind, "rows replaced:", replaced, "of", K * ROWS)
    assert replaced >= 1                                    # the polish did something
    assert (want_f <= a["fitness"]).all()                   # no fitness rose
    assert b["population"].tobytes() == want_p.tobytes()
    assert b["fitness"].tobytes() == want_f.tobytes()


def test_the_best_so_far_follows_an_improved_top_row(states):
    kind, a, b, _ = states
    improved = 0
    for k in range(K):
        top = int(np.argmin(b["fitness"][k]))
        if float(b["fitness"][k, top]) + 1e-10 < a["best_fit"][k]:
            improved += 1
            assert b["best"][k].tobytes() == b["population"][k, top].tobytes(), k
            assert b["best_fit"][k] == float(b["fitness"][k, top]), k
        else:
            assert b["best"][k].tobytes() == a["best"][k].tobytes() and b["best_fit"][k] == a["best_fit"][k], k
    assert improved >= 1
    assert b["curves"] == a["curves"]                       # written before the polish: untouched


def test_breeding_continues_from_the_polished_rows(states):
    kind, _, b, b2 = states
    (fresh,) = _run(kind, b["population"], [(G + 1, 2)])
    assert b2["population"].tobytes() != b["population"].tobytes()
    _same(b2, fresh, "two generations after the polish", keys=("population", "fitness"))
    # the fresh group evaluated the polished rows itself: the installed fitness is the row's own
    (again,) = _run(kind, b["population"], [(G + 1, 0)])
    assert again["fitness"].tobytes() == b["fitness"].tobytes()


def test_a_migration_and_a_polish_on_the_same_generation(states):
    kind, a, _, _ = states
    pops = _problem()[3]
    (b,) = _run(kind, pops, [(1, G)], every_mig=G, mig=2, polish=_on())
    mig_p, mig_f = ga.ring_migration(a["population"], a["fitness"], 2,
                                     refit=_refit if kind == "per_island" else None)
    want_p, want_f = ga.polish_elites(mig_p, mig_f, ROWS, _refine(kind))
    assert b["population"].tobytes() == want_p.tobytes()
    assert b["fitness"].tobytes() == want_f.tobytes()


def _digest(st):
    return dict(population=st["population"], fitness=st["fitness"], best=st["best"], best_fit=st["best_fit"],
                curves=np.asarray([[c["best"], c["mean"], c["median"]] for c in st["curves"]]))


def _off(g):
    g.set_polish(G, STEPS, ROWS)
    g.clear_polish()


@pytest.mark.parametrize("polish", [lambda g: g.set_polish(0, STEPS, ROWS), lambda g: g.set_polish(G, 0, ROWS), _off,
                                    lambda g: g.set_polish(1000, STEPS, ROWS)],
                         ids=["every_0", "steps_0", "null", "never_reached"])
def test_off_is_off(polish, states):
    kind = states[0]
    pops = _problem()[3]
    if ("plain", kind) not in _cache:
        _cache["plain", kind] = _digest(_run(kind, pops, [(1, G + 2)], every_mig=2, mig=1)[0])
    got = _digest(_run(kind, pops, [(1, G + 2)], every_mig=2, mig=1, polish=polish)[0])
    for key, v in _cache["plain", kind].items():
        assert got[key].tobytes() == v.tobytes(), key


def test_a_polish_that_improves_nothing_installs_nothing(states):
    """Zero learning rates: every candidate's best is its start at the row's own
    fitness, which is not strictly lower, so no row, elite list or best changes."""
    kind, a, _, _ = states
    pops = _problem()[3]
    (b,) = _run(kind, pops, [(1, G)], polish=lambda g: g.set_polish(G, STEPS, ROWS, lr=[0.0] * 9))
    _same(b, a, "a polish with zero rates")
    assert b["curves"] == a["curves"]


def test_a_setting_holds_for_the_generations_run_after_it(states):
    """Generation G has run and is not yet closed when the setting changes: it is
    closed under the setting it ran with."""
    kind, a, b, _ = states
    pops = _problem()[3]
    g = _group(kind, pops)
    try:
        g.run(1, G, TOTAL)
        g.set_polish(G, STEPS, ROWS)          # too late for generation G
        _same(g.read(), a, "set_polish after the run")
    finally:
        g.close()
    g = _group(kind, pops, polish=_on())
    try:
        g.run(1, G, TOTAL)
        g.clear_polish()                      # generation G ran with the polish on
        _same(g.read(), b, "clear_polish after the run")
    finally:
        g.close()


def test_bad_polish_parameters_leave_the_session_as_it_was():
    pops = _problem()[3]
    g = _group("shared", pops)
    try:
        for args in ((2, 3, 0), (2, 3, ELITE + 1), (-1, 3, 1), (2, -1, 1)):
            with pytest.raises(ggs.GGSInputError):
                g.set_polish(*args)
        with pytest.raises(ggs.GGSInputError):
            g.set_polish(2, 3, 1, beta1=1.0)
        g.run(1, G, TOTAL)
        got = g.read()
    finally:
        g.close()
    (plain,) = _run("shared", pops, [(1, G)])
    _same(got, plain, "after refused set_polish calls")


def _unfused_case():
    pops = _problem()[3]
    (end,) = _run("per_island", pops, [(1, 5)], every_mig=4, mig=1, polish=_on(every=2))
    return end


_UNFUSED_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import test_gpu_memetic as T
np.savez(sys.argv[3], **T._digest(T._unfused_case()))
"""


def test_ga_unfused_gives_the_same_bits(tmp_path):
    """The switch is read once per process: a fresh child."""
    pkg = os.path.dirname(os.path.dirname(ggs.__file__))
    path = str(tmp_path / "unfused.npz")
    subprocess.run([sys.executable, "-c", _UNFUSED_SCRIPT, pkg, os.path.dirname(__file__), path], check=True,
                   timeout=300, env=dict(os.environ, GGS_GA_UNFUSED="1"))
    want = _digest(_unfused_case())
    un = np.load(path)
    for key, v in want.items():
        np.testing.assert_array_equal(un[key], v, err_msg=key)


@pytest.mark.parametrize("kind", ["shared", "per_island"])
def test_a_group_of_one(kind):
    pops = _problem()[3][:1]
    (plain,) = _run(kind, pops, [(1, 6)], seeds=SEEDS[:1])
    (st,) = _run(kind, pops, [(1, 6)], seeds=SEEDS[:1], polish=_on(every=2, rows=1))
    best = st["curves"][0]["best"]
    assert all(y <= x for x, y in zip(best, best[1:]))
    assert st["best_fit"][0] <= best[-1]                    # a polish after the last row can only lower it
    print(kind, "K = 1: plain", plain["best_fit"][0], "memetic", st["best_fit"][0])
    assert np.isfinite(st["fitness"]).all() and st["best_fit"][0] <= float(st["fitness"][0].min())


# ---- the Python drivers ----------------------------------------------------------------
def _driver_kw():
    zero = dict.fromkeys(("xy", "alog", "blog", "theta", "rgb", "alpha"), 0.0)
    smax = dict(xy=0.05, alog=0.2, blog=0.2, theta=0.3, rgb=20.0, alpha=20.0)
    return dict(pop_size=8, n_splats=12, generations=4, tour_k=2, elite_k=1, cxpb=0.5, mutpb=0.3,
                mut_sigma_max=smax, mut_sigma_min=zero, schedule="linear", min_scale_splats=0.5,
                max_scale_splats=0.5, k_sigma=3.0, mask_strength=0.5, boost_only=False, progress=False)


def test_genetic_approx_memetic_is_no_worse():
    img = np.random.default_rng(5).uniform(0, 255, (32, 32, 3)).astype(np.uint8)
    kw = dict(_driver_kw(), seed=9, backend="device")
    _, f0 = ga.genetic_approx(img, 48, 48, None, **kw)
    best, f1 = ga.genetic_approx(img, 48, 48, None, memetic_every=2, memetic_steps=3, **kw)
    print("GA best", f0, "memetic", f1)
    assert f1 <= f0 and best.shape == (12, 9)
    # the island group of one without a polish reached is the single session
    _, f2 = ga.genetic_approx(img, 48, 48, None, memetic_every=1000, memetic_steps=3, **kw)
    assert f2 == f0


def test_genetic_approx_many_polish_is_genetic_approx_per_image():
    images = [np.random.default_rng(70 + k).uniform(0, 255, (32, 32, 3)).astype(np.uint8) for k in range(2)]
    kw = _driver_kw()
    many = ga.genetic_approx_many(images, 48, 48, None, seed=9, polish_steps=5, **kw)
    plain = ga.genetic_approx_many(images, 48, 48, None, seed=9, **kw)
    assert any(many[k][1] < plain[k][1] for k in range(2))  # the polish improved something
    for k in range(2):
        b, f = ga.genetic_approx(images[k], 48, 48, None, seed=9 + k, backend="device", polish_steps=5, **kw)
        assert many[k][0].tobytes() == b.tobytes() and many[k][1] == f, k
