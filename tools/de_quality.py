"""Best fitness of the device GA and the device DE after the same number of
candidate evaluations, at the reference's shipped GA shape (512x512, 512 splats,
pop 32, weighted fitness) on a seeded synthetic target.  The GA (elite 8) spends
24 evaluations per generation, DE 32; the initial population's 32 count for both.
The GA's sigma schedule runs over each budget's own generation count, so it gets
one run per budget; DE has no schedule and is read at each budget of one run.
Prints one JSON line per (seed, budget) and a summary line.

usage: python tools/de_quality.py [--budgets 240000 1200000] [--seeds 1 2 3]"""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "genetic-gaussian-splats_amd"))
from ggs import ga
from ggs.ga_device import DeviceDE, DeviceGA
from ggs.mask import compute_importance_mask, prepare_target

ap = argparse.ArgumentParser()
ap.add_argument("--budgets", type=int, nargs="+", default=[240000, 1200000])
ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
ap.add_argument("--strategy", default="rand1")
ap.add_argument("--crossover", default="gene")
ap.add_argument("--F", type=float, nargs=2, default=[0.5, 0.9])
ap.add_argument("--CR", type=float, default=0.3)
a = ap.parse_args()
H = W = 512
N, P, E = 512, 32, 8
cfg = dict(mut_sigma_max={"xy": 0.1, "alog": 0.5, "blog": 0.5, "theta": 0.3, "rgb": 25.0, "alpha": 25.0},
           mut_sigma_min={"xy": 0.01, "alog": 0.05, "blog": 0.05, "theta": 0.025, "rgb": 2.0, "alpha": 2.0},
           schedule="cosine")
target = np.random.default_rng(0).uniform(0, 255, (H + 9, W + 5, 3)).astype(np.float32)
t = prepare_target(target, H, W)
m = compute_importance_mask(t, H, W, smooth=3, strength=0.7)
budgets = sorted(a.budgets)
rows = []
for seed in a.seeds:
    init = ga.new_population(P, N, H, W, 3.0, 0.1, np.random.default_rng(seed))
    dde = DeviceDE(t, m, init, strategy=a.strategy, crossover=a.crossover, F=tuple(a.F), CR=a.CR,
                   min_scale_splats=3.0, max_scale_splats=0.1, seed=seed)
    gen, de_fit = 1, {}
    for b in budgets:
        g = (b - P) // P
        dde.run(gen, g + 1 - gen)
        gen = g + 1
        de_fit[b] = dde.read()["best_fit"]
    f0 = dde.read()["curves"]["best"][0]
    dde.close()
    for b in budgets:
        g = (b - P) // (P - E)
        dga = DeviceGA(t, m, init, tour_k=2, elite_k=E, cxpb=0.05, mutpb=0.05, min_scale_splats=3.0,
                       max_scale_splats=0.1, seed=seed, **cfg)
        dga.run(1, g, g)
        row = {"seed": seed, "evaluations": b, "initial_best": f0, "ga_generations": g,
               "ga_best": dga.read()["best_fit"], "de_generations": (b - P) // P, "de_best": de_fit[b]}
        dga.close()
        rows.append(row)
        print(json.dumps(row), flush=True)
summary = {str(b): {"ga_mean": float(np.mean([r["ga_best"] for r in rows if r["evaluations"] == b])),
                    "de_mean": float(np.mean([r["de_best"] for r in rows if r["evaluations"] == b]))}
           for b in budgets}
print(json.dumps({"metric": "best fitness after equal candidate evaluations", "summary": summary,
                  "config": {"H": H, "W": W, "splats": N, "pop": P, "ga_elite": E, "strategy": a.strategy,
                             "crossover": a.crossover, "F": a.F, "CR": a.CR}}))
