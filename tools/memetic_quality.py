"""Memetic island GA against the GA alone and against a final polish, at equal wall
time: the reference's shipped GA shape (512x512, 512 splats, pop 32, elite 8,
weighted fitness) on tools/de_quality.py's seeded noise target.

  (a) the GA alone for --wall seconds' worth of generations;
  (b) 80 % of those generations, then Adam steps on every island's best individual
      (one refine session) for the remaining fifth of the time;
  (c) memetic runs over every x steps x rows, the generation count chosen so that
      generations plus polish events fill the same wall time.

Every run's sigma schedule spans its own generation count.  Rates (generations/s,
refine steps/s, seconds per polish event) are calibrated per process on short runs
first; each row states the wall time the run really took.  With --cost the cost of
one polish event at rows = 1, steps = 5 is measured instead (a synchronised run of
--events generations with every = 1 against the same run without, per event: the
host clock, so the figure also holds what every generation loses by being closed
unfused before its polish), beside --islands solo B = 1 refine sessions doing the
same steps.
Prints one JSON line per run and a summary line.

usage: python tools/memetic_quality.py [--islands 1] [--wall 5] [--seeds 1 2 3] [--cost]"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "genetic-gaussian-splats_amd"))
from ggs import ga
from ggs.ga_device import DeviceGAIslands, DeviceRefine
from ggs.mask import compute_importance_mask, prepare_target
from ggs.refine import DEFAULT_LR

ap = argparse.ArgumentParser()
ap.add_argument("--islands", type=int, default=1)
ap.add_argument("--wall", type=float, default=5.0)
ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
ap.add_argument("--every", type=int, nargs="+", default=[200, 1000])
ap.add_argument("--steps", type=int, nargs="+", default=[5, 20])
ap.add_argument("--rows", type=int, nargs="+", default=[1, 4])
ap.add_argument("--cost", action="store_true")
ap.add_argument("--events", type=int, default=200)
a = ap.parse_args()
H = W = 512
N, P, E, K = 512, 32, 8, a.islands
cfg = dict(mut_sigma_max={"xy": 0.1, "alog": 0.5, "blog": 0.5, "theta": 0.3, "rgb": 25.0, "alpha": 25.0},
           mut_sigma_min={"xy": 0.01, "alog": 0.05, "blog": 0.05, "theta": 0.025, "rgb": 2.0, "alpha": 2.0},
           schedule="cosine")
target = np.random.default_rng(0).uniform(0, 255, (H + 9, W + 5, 3)).astype(np.float32)
t = prepare_target(target, H, W)
m = compute_importance_mask(t, H, W, smooth=3, strength=0.7)


def pops_of(seed):
    return np.stack([ga.new_population(P, N, H, W, 3.0, 0.1, np.random.default_rng(seed + k)) for k in range(K)])


def group(seed, polish=None):
    g = DeviceGAIslands(t, m, pops_of(seed), [seed + k for k in range(K)], 0, 0, tour_k=2, elite_k=E, cxpb=0.05,
                        mutpb=0.05, min_scale_splats=3.0, max_scale_splats=0.1, **cfg)
    if polish:
        g.set_polish(*polish)
    return g


def run_group(seed, gens, polish=None):
    """(state, seconds) of `gens` generations, the read's synchronisation included."""
    g = group(seed, polish)
    try:
        t0 = time.perf_counter()
        g.run(1, gens, gens)
        st = g.read()
        return st, time.perf_counter() - t0
    finally:
        g.close()


def refine_best(genomes, steps):
    """(best_fits [B], seconds) of `steps` Adam steps on [B,N,9] in one session."""
    s = DeviceRefine(t, m, genomes, lr=DEFAULT_LR, min_scale_splats=3.0, max_scale_splats=0.1)
    try:
        t0 = time.perf_counter()
        s.run(steps)
        r = s.read()
        return r["best_fits"], time.perf_counter() - t0
    finally:
        s.close()


run_group(0, 500)                                        # warm-up: allocations, code objects
_, sec = run_group(0, 4000)
gen_rate = 4000 / sec
_, sec = refine_best(pops_of(0)[:, 0], 200)
step_rate = 200 / sec
if a.cost:
    n = a.events
    _, plain = run_group(0, n)
    _, with_p = run_group(0, n, (1, 5, 1))
    per_event = (with_p - plain) / n
    solo = 0.0
    for k in range(K):
        _, s1 = refine_best(pops_of(0)[k:k + 1, 0], 5)
        solo += s1
    print(json.dumps({"metric": "cost of one polish event", "islands": K, "rows": 1, "steps": 5, "events": n,
                      "ms_per_event": 1e3 * per_event, "ms_solo_sessions": 1e3 * solo,
                      "generations_per_s": gen_rate, "generations_displaced": per_event * gen_rate,
                      "timing": "host clock around a synchronised run, per event; includes the generation's unfused close"}))
    sys.exit(0)

G_a = int(gen_rate * a.wall)
rows = []


def emit(row):
    rows.append(row)
    print(json.dumps(row), flush=True)


grid = [(e, s, r) for e in a.every for s in a.steps for r in a.rows]
event_sec = {}
for e, s, r in grid:                                     # seconds per polish event, from ten events
    _, with_p = run_group(0, 10 * e, (e, s, r))
    event_sec[e, s, r] = max((with_p - 10 * e / gen_rate) / 10, 0.0)
for seed in a.seeds:
    st, sec = run_group(seed, G_a)
    emit({"seed": seed, "islands": K, "run": "ga", "generations": G_a, "best": float(st["best_fit"].min()),
          "wall_s": sec})
    G_b = int(0.8 * G_a)
    st, sec = run_group(seed, G_b)
    n_steps = max(int(step_rate * 0.2 * a.wall), 1)
    bf, sec2 = refine_best(st["best"], n_steps)
    emit({"seed": seed, "islands": K, "run": "ga80+polish", "generations": G_b, "adam_steps": n_steps,
          "ga_best": float(st["best_fit"].min()), "best": float(min(bf.min(), st["best_fit"].min())),
          "wall_s": sec + sec2})
    for e, s, r in grid:
        G_c = int(a.wall / (1.0 / gen_rate + event_sec[e, s, r] / e))
        st, sec = run_group(seed, G_c, (e, s, r))
        emit({"seed": seed, "islands": K, "run": "memetic", "every": e, "steps": s, "rows": r, "generations": G_c,
              "best": float(st["best_fit"].min()), "wall_s": sec})


def mean(sel):
    v = [x["best"] for x in rows if sel(x)]
    return float(np.mean(v)) if v else None


summary = {"ga": mean(lambda x: x["run"] == "ga"), "ga80+polish": mean(lambda x: x["run"] == "ga80+polish")}
for e, s, r in grid:
    summary[f"memetic every={e} steps={s} rows={r}"] = mean(
        lambda x: x["run"] == "memetic" and (x["every"], x["steps"], x["rows"]) == (e, s, r))
print(json.dumps({"metric": "best fitness at equal wall time (mean over seeds)", "islands": K, "wall_s": a.wall,
                  "generations_per_s": gen_rate, "refine_steps_per_s": step_rate, "summary": summary,
                  "config": {"H": H, "W": W, "splats": N, "pop": P, "elite": E}}))
