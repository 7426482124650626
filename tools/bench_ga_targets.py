"""Island groups with a target per island: island-generations/s on the shipped GA
shape (512x512, 512 splats, pop 32, elite 8, tour 2; run_ggs.py:41 with
modules/config.py:5-11), K islands, no migration unless asked.

--mode targets  one DeviceGAIslands group, K distinct targets (ggs_ga_islands_create_targets)
--mode shared   the same group on one shared target (ggs_ga_islands_create; also runs
                on an older library: GGS_LIB=libggs_<rev>.so)
--mode solo     K DeviceGA sessions one after the other (what a folder of images
                costs without the group)
Each mode: 5 warm-up generations, then --gens timed generations ending in a read
(a device sync), --repeats times in one process; one JSON line with every repeat.

usage: python tools/bench_ga_targets.py --mode targets [--islands 8] [--gens 300] [--repeats 3]"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "genetic-gaussian-splats_amd"))
import ggs
from ggs import ga
from ggs.ga_device import DeviceGA, DeviceGAIslands
from ggs.mask import compute_importance_mask, prepare_target

ap = argparse.ArgumentParser()
ap.add_argument("--mode", required=True, choices=["targets", "shared", "solo"])
ap.add_argument("--islands", type=int, default=8)
ap.add_argument("--gens", type=int, default=300)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--splats", type=int, default=512)
ap.add_argument("--pop", type=int, default=32)
ap.add_argument("--elite", type=int, default=8)
ap.add_argument("--migrate-every", type=int, default=0)
ap.add_argument("--migrants", type=int, default=0)
a = ap.parse_args()
K, H, W, G = a.islands, a.size, a.size, a.gens
cfg = dict(mut_sigma_max={"xy": 0.1, "alog": 0.5, "blog": 0.5, "theta": 0.3, "rgb": 25.0, "alpha": 25.0},
           mut_sigma_min={"xy": 0.01, "alog": 0.05, "blog": 0.05, "theta": 0.025, "rgb": 2.0, "alpha": 2.0},
           schedule="cosine", tour_k=2, elite_k=a.elite, cxpb=0.05, mutpb=0.05, min_scale_splats=3.0,
           max_scale_splats=0.1)
t = np.stack([prepare_target(np.random.default_rng(k).uniform(0, 255, (H, W, 3)).astype(np.float32), H, W)
              for k in range(K)])
m = np.stack([compute_importance_mask(x, H, W, smooth=3, strength=0.7) for x in t]).astype(np.float32)
init = np.stack([ga.new_population(a.pop, a.splats, H, W, 3.0, 0.1, np.random.default_rng(k)) for k in range(K)])
seeds = [1 + k for k in range(K)]


def timed(session):
    session.run(1, 5, G + 5)                      # warm-up
    session.read()
    t0 = time.perf_counter()
    session.run(6, G, G + 5)
    st = session.read()
    return time.perf_counter() - t0, float(np.min(st["best_fit"]))


times, best = [], None
for _ in range(a.repeats):
    if a.mode == "solo":
        dt = 0.0
        for k in range(K):
            s = DeviceGA(t[k], m[k], init[k], seed=seeds[k], **cfg)
            try:
                d, best = timed(s)
                dt += d
            finally:
                s.close()
    else:
        tt, mm = (t, m) if a.mode == "targets" else (t[0], m[0])
        s = DeviceGAIslands(tt, mm, init, seeds, a.migrate_every, a.migrants, **cfg)
        try:
            dt, best = timed(s)
        finally:
            s.close()
    times.append(dt)
rates = [K * G / d for d in times]
print(json.dumps({"metric": "island-generations/s", "mode": a.mode, "lib": os.path.basename(ggs.LIB_PATH),
                  "value": round(float(np.median(rates)), 1), "repeats": [round(r, 1) for r in rates],
                  "ms_per_group_generation": round(1e3 * float(np.median(times)) / G, 4),
                  "config": {"H": H, "W": W, "splats": a.splats, "pop": a.pop, "elite": a.elite, "islands": K,
                             "gens": G, "migrate_every": a.migrate_every, "migrants": a.migrants},
                  "best_fit": best}))
