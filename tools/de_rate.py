"""DE generations/s against the GA's device loop, same process, same device, at the
reference's shipped GA shape (512x512, 512 splats, pop 32, weighted fitness; the GA
with elite 8, so it rasterises 24 candidates per generation where DE rasterises 32).

The two loops are timed in alternating windows (each a run of --gens generations
that ends in a read, i.e. a device sync) after a warm-up of both; then one
HIP-event profiled run of each gives the per-launch device time of variation
("prep"), raster and select.  Prints one JSON line.

usage: python tools/de_rate.py [--gens 4000] [--repeats 3] [--profile-gens 500]"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "genetic-gaussian-splats_amd"))
import ggs
from ggs import ga
from ggs.ga_device import DeviceDE, DeviceGA
from ggs.mask import compute_importance_mask, prepare_target

ap = argparse.ArgumentParser()
ap.add_argument("--gens", type=int, default=4000)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--profile-gens", type=int, default=500)
ap.add_argument("--strategy", default="rand1")
ap.add_argument("--crossover", default="gene")
a = ap.parse_args()
H = W = 512
N, P, E = 512, 32, 8
cfg = dict(mut_sigma_max={"xy": 0.1, "alog": 0.5, "blog": 0.5, "theta": 0.3, "rgb": 25.0, "alpha": 25.0},
           mut_sigma_min={"xy": 0.01, "alog": 0.05, "blog": 0.05, "theta": 0.025, "rgb": 2.0, "alpha": 2.0},
           schedule="cosine")
target = np.random.default_rng(0).uniform(0, 255, (H, W, 3)).astype(np.float32)
t = prepare_target(target, H, W)
m = compute_importance_mask(t, H, W, smooth=3, strength=0.7)
init = ga.new_population(P, N, H, W, 3.0, 0.1, np.random.default_rng(0))
total = 5 + a.gens * a.repeats + a.profile_gens
dga = DeviceGA(t, m, init, tour_k=2, elite_k=E, cxpb=0.05, mutpb=0.05, min_scale_splats=3.0,
               max_scale_splats=0.1, seed=1, **cfg)
dde = DeviceDE(t, m, init, strategy=a.strategy, crossover=a.crossover, min_scale_splats=3.0,
               max_scale_splats=0.1, seed=1)
loops = {"ga": lambda g, n: dga.run(g, n, total), "de": lambda g, n: dde.run(g, n)}
reads = {"ga": dga.read, "de": dde.read}
gen = {"ga": 1, "de": 1}


def window(name, n):
    t0 = time.perf_counter()
    loops[name](gen[name], n)
    reads[name]()                                                  # synchronises
    gen[name] += n
    return n / (time.perf_counter() - t0)


for name in ("ga", "de"):
    window(name, 5)                                                # warm-up
rates = {"ga": [], "de": []}
for _ in range(a.repeats):
    for name in ("ga", "de"):
        rates[name].append(round(window(name, a.gens), 1))
kern = {}
for name in ("ga", "de"):                                          # events add host work: not the rate
    ggs.profile_reset()
    ggs.profile_enable(True)
    window(name, a.profile_gens)
    ggs.profile_enable(False)
    kern[name] = {k + "_us": round(ms * 1e3 / max(n, 1), 2)
                  for k, (ms, n) in ((k, ggs.profile_read(k)) for k in ("prep", "raster", "finalize", "select"))
                  if n}
med = {k: float(np.median(v)) for k, v in rates.items()}
print(json.dumps({"metric": "DE generations/s (device-resident)", "value": med["de"],
                  "ga_generations_per_s": med["ga"], "de_over_ga_time": round(med["ga"] / med["de"], 4),
                  "expected_time_ratio_P_over_P_minus_E": round(P / (P - E), 4), "windows": rates,
                  "device_us_per_launch": kern,
                  "config": {"H": H, "W": W, "splats": N, "pop": P, "ga_elite": E, "gens": a.gens,
                             "strategy": a.strategy, "crossover": a.crossover},
                  "best_fit": {"ga": reads["ga"]()["best_fit"], "de": reads["de"]()["best_fit"]}}))
dga.close()
dde.close()
