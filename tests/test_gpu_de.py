"""The device-resident differential evolution (ggs_de_*, ga_device.DeviceDE) on an
MI355X, held bit for bit to the numpy statement ggs/de.py on the Philox draws
restated in tests/_philox_de.py:

* one generation: the trials are ``de_trials`` of the state read before it, and
  population, fitness, best and the curves row are ``de_select`` plus the stats;
* a trial's fitness is the product's fitness of that genome, in the three modes;
* a run — whole or in chunks, with a parameter switch, beside another session on
  another thread — is the host loop's trajectory;
* ``differential_evolution`` on the device writes its frames and CSV.
"""
from __future__ import annotations

import csv
import os
import threading

import numpy as np
import pytest

import _philox_de as XD
import ggs
from ggs import de, ga
from ggs.ga_device import DeviceDE
from test_gpu_ga import _problem

pytestmark = pytest.mark.gpu
# test_gpu_ga_philox.py's scale bounds: the log-scale clip interval is not empty on small canvases
MIN_S, MAX_S = 0.5, 0.5
SEEDS = (0, 2**63 + 12345)
F, CR = (0.5, 0.9), 0.3


def _session(t, m, init, seed, strategy, crossover, boost=False, F=F, CR=CR):
    return DeviceDE(t, m, init, strategy=strategy, crossover=crossover, F=F, CR=CR, min_scale_splats=MIN_S,
                    max_scale_splats=MAX_S, boost_only=boost, seed=seed)


def _host_kw(H, W, strategy, crossover, F=F, CR=CR):
    lo, hi = ga.scale_log_bounds(H, W, MIN_S, MAX_S)
    return dict(strategy=strategy, crossover=crossover, f_lo=F[0], f_hi=F[1], cr=CR, log_lo=lo, log_hi=hi)


def _same_state(a, b, what):
    for k in ("population", "fitness", "best"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")
    assert a["best_fit"] == b["best_fit"], what
    for k in ("best", "mean", "median"):
        assert a["curves"][k] == b["curves"][k], (what, k)


@pytest.mark.parametrize("P,N,H,W", [
    (4, 1, 16, 16),          # minimum P: every index draw is shifted; jrand with one splat
    (5, 37, 33, 47),         # odd P, N no multiple of 64, canvas no multiple of the strip
    (12, 1100, 40, 24),      # several splats per thread
    (512, 2, 16, 16),        # the population limit
])
@pytest.mark.parametrize("strategy", sorted(de.STRATEGIES))
@pytest.mark.parametrize("crossover", sorted(de.CROSSOVERS))
def test_one_generation_is_the_numpy_statement(P, N, H, W, strategy, crossover):
    _, t, m = _problem(H, W, N)
    init = ga.new_population(P, N, H, W, MIN_S, MAX_S, np.random.default_rng(N))
    kw = _host_kw(H, W, strategy, crossover)
    for seed in SEEDS:
        s = _session(t, m, init, seed, strategy, crossover)
        try:
            s0 = s.read()
            np.testing.assert_array_equal(s0["population"], init)
            g, mean, med = de.de_stats(s0["fitness"])
            assert s0["curves"] == {"best": [float(s0["fitness"][g])], "mean": [mean], "median": [med]}
            assert s0["best_fit"] == float(s0["fitness"][g])
            np.testing.assert_array_equal(s0["best"], init[g])
            for gen in (1, 1000):
                s.run(gen, 1)
                s1 = s.read()
                d = XD.draws(seed, gen, P, N, crossover == "splat")
                trials = de.de_trials(s0["population"], s0["fitness"], d, **kw)
                np.testing.assert_array_equal(s1["trials"], trials, err_msg=f"trials, seed {seed} gen {gen}")
                assert not np.array_equal(trials, s0["population"])
                pop, fits = de.de_select(s0["population"], s0["fitness"], s1["trials"], s1["trial_fits"])
                np.testing.assert_array_equal(s1["population"], pop)
                np.testing.assert_array_equal(s1["fitness"], fits)
                g, mean, med = de.de_stats(fits)
                best, best_fit = s0["best"], s0["best_fit"]
                if float(fits[g]) + 1e-10 < best_fit:
                    best, best_fit = pop[g], float(fits[g])
                np.testing.assert_array_equal(s1["best"], best)
                assert s1["best_fit"] == best_fit
                for k, v in (("best", best_fit), ("mean", mean), ("median", med)):
                    assert s1["curves"][k] == s0["curves"][k] + [v], (k, seed, gen)
                s0 = s1
        finally:
            s.close()


@pytest.mark.parametrize("mode", ["none", "weighted", "boost"])
def test_trial_fitness_is_the_products_fitness(mode):
    P, N, H, W = 8, 37, 33, 47
    _, t, m = _problem(H, W, 5)
    mask = None if mode == "none" else m
    boost = mode == "boost"
    init = ga.new_population(P, N, H, W, MIN_S, MAX_S, np.random.default_rng(5))
    s = _session(t, mask, init, 7, "rand1", "gene", boost=boost)
    try:
        s.run(1, 3)
        st = s.read()
    finally:
        s.close()
    np.testing.assert_array_equal(st["trial_fits"],
                                  ggs.fitness(st["trials"], t, H, W, 3.0, weight_mask=mask, boost_only=boost))
    np.testing.assert_array_equal(st["fitness"],
                                  ggs.fitness(st["population"], t, H, W, 3.0, weight_mask=mask, boost_only=boost))
    assert float(ggs.fitness(st["best"][None], t, H, W, 3.0, weight_mask=mask, boost_only=boost)[0]) == st["best_fit"]


@pytest.mark.parametrize("boost", [False, True])
@pytest.mark.parametrize("strategy,crossover", [("rand1", "gene"), ("best1", "splat"), ("current-to-best1", "gene")])
def test_device_run_is_the_host_loop(strategy, crossover, boost):
    P, N, H, W, G = 16, 24, 32, 32, 8
    seed = 2**63 + 12345
    target, t, m = _problem(H, W, 3)
    init = ga.new_population(P, N, H, W, MIN_S, MAX_S, np.random.default_rng(3))
    hb, hf, hs = de.differential_evolution(
        target, H, W, "cuda", P, N, G, strategy=strategy, crossover=crossover, F=F, CR=CR, min_scale_splats=MIN_S,
        max_scale_splats=MAX_S, k_sigma=3.0, mask_strength=0.7, boost_only=boost, init_population=init,
        progress=False, return_state=True, backend="host", draws=XD.PhiloxDeDraws(seed, crossover))
    host = dict(hs, best=hb, best_fit=hf)
    assert len(hs["curves"]["best"]) == G + 1 and hs["curves"]["best"][-1] < hs["curves"]["best"][0]
    for chunks in ([8], [3, 3, 2]):
        s = _session(t, m, init, seed, strategy, crossover, boost=boost)
        try:
            gen = 1
            for n in chunks:
                s.run(gen, n)
                gen += n
            _same_state(s.read(), host, f"chunks {chunks}")
        finally:
            s.close()


def test_set_params_between_runs_is_the_host_loop_with_the_same_switch():
    P, N, H, W = 16, 24, 32, 32
    seed = 42
    _, t, m = _problem(H, W, 4)
    init = ga.new_population(P, N, H, W, MIN_S, MAX_S, np.random.default_rng(4))
    a = dict(strategy="rand1", crossover="gene", F=(0.5, 0.9), CR=0.3)
    b = dict(strategy="current-to-best1", crossover="splat", F=(0.7, 0.7), CR=0.9)

    def evaluate(g):
        return ggs.fitness(g, t, H, W, 3.0, weight_mask=m)

    st = de.run_host_de(init, 3, XD.PhiloxDeDraws(seed, a["crossover"]), evaluate,
                        **_host_kw(H, W, a["strategy"], a["crossover"], a["F"], a["CR"]))
    st = de.run_host_de(None, 3, XD.PhiloxDeDraws(seed, b["crossover"]), evaluate, first_gen=4, state=st,
                        **_host_kw(H, W, b["strategy"], b["crossover"], b["F"], b["CR"]))
    s = _session(t, m, init, seed, a["strategy"], a["crossover"], F=a["F"], CR=a["CR"])
    try:
        s.run(1, 3)
        s.set_params(**b)
        s.run(4, 3)
        got = s.read()
        with pytest.raises(AssertionError):
            s.set_params(strategy="rand1", crossover="gene", F=(0.9, 0.5), CR=0.3)
    finally:
        s.close()
    _same_state(got, st, "switch")
    np.testing.assert_array_equal(got["trials"], st["trials"])
    np.testing.assert_array_equal(got["trial_fits"], st["trial_fits"])


def test_two_sessions_on_two_threads_each_equal_their_solo_run():
    """Each session has its own stream, workspace and finalize counters (512^2 folds
    the finalize into the raster, 96 x 80 does not)."""
    shapes = [(512, 512, 128, 24, 1), (96, 80, 40, 48, 2)]

    def run(H, W, N, P, seed):
        _, t, m = _problem(H, W, seed)
        init = ga.new_population(P, N, H, W, MIN_S, MAX_S, np.random.default_rng(seed))
        s = _session(t, m, init, seed, "current-to-best1", "gene")
        try:
            s.run(1, 12)
            return s.read()
        finally:
            s.close()

    solo = [run(*sh) for sh in shapes]
    got = [None] * len(shapes)

    def worker(i):
        got[i] = run(*shapes[i])
    th = [threading.Thread(target=worker, args=(i,)) for i in range(len(shapes))]
    for x in th:
        x.start()
    for x in th:
        x.join(300)
    for a, b in zip(got, solo):
        assert a is not None
        _same_state(a, b, "concurrent")


def test_differential_evolution_on_the_device_writes_frames_and_csv(tmp_path):
    P, N, H, W, G = 12, 20, 32, 32, 8
    target, t, m = _problem(H, W, 6)
    frames = tmp_path / "frames"
    frames.mkdir()
    path = tmp_path / "out" / "loss.csv"
    kw = dict(min_scale_splats=MIN_S, max_scale_splats=MAX_S, k_sigma=3.0, mask_strength=0.7, boost_only=False,
              seed=9, progress=False, return_state=True)
    b, f, st = de.differential_evolution(target, H, W, "cuda", P, N, G, save_video=True, frame_every=4,
                                         video_dir=str(frames), loss_csv_path=str(path), chunk=3, **kw)
    assert sorted(os.listdir(frames)) == ["de_0.png", "de_4.png", "de_8.png"]
    with open(path) as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == ["gen", "best", "mean", "median"] and len(rows) == G + 2
    assert [float(r[1]) for r in rows[1:]] == st["curves"]["best"]
    c = st["curves"]["best"]
    assert all(y <= x for x, y in zip(c, c[1:])) and f == c[-1]
    assert float(ggs.fitness(b[None], t, H, W, 3.0, weight_mask=m)[0]) == f
    # the frames and the chunking change nothing
    b2, f2, st2 = de.differential_evolution(target, H, W, "cuda", P, N, G, backend="device", chunk=50, **kw)
    _same_state(dict(st, best=b, best_fit=f), dict(st2, best=b2, best_fit=f2), "chunking")
