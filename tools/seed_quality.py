"""Seeding from the target measured: what it costs and what it does.

  --cost    at the shipped shape (512x512, 512 splats), K = 1 and 8 images: the device time of
            one placement (cell, rank, apply) per cell size and of one full seeding with the
            default schedule, from the library's own HIP events (ggs_profile_read("seed")),
            beside one render call ("prep" + "raster") and one refine step (host clock around
            run(--steps) and a synchronising read) measured in the same run.
  (default) fitness at the start and after equal refine steps and equal GA generations, from
            a seeded start (``seeded_population`` of the seeded genome) and from
            ``new_population``, same seeds for both, on a structured synthetic target (the
            render of a hidden random genome mixed with a gradient) and on the noise target
            of tools/de_quality.py and tools/density_quality.py.
  --sweep   the seeded genome's own fitness on both targets when the default schedule's sigma
            are replaced by cell / d and alpha for a small grid,
            and when the rounds start one cell size finer.
Prints one JSON line per measurement and a summary line.

usage: python tools/seed_quality.py [--cost | --sweep] [--seeds 1 2 3] [--steps N] [--generations G]"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "genetic-gaussian-splats_amd"))
import ggs
from ggs import api, ga
from ggs import seed as S
from ggs.ga_device import DeviceGA, DeviceRefine
from ggs.mask import compute_importance_mask, prepare_target
from ggs.refine import DEFAULT_LR

ap = argparse.ArgumentParser()
ap.add_argument("--cost", action="store_true")
ap.add_argument("--sweep", action="store_true")
ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
ap.add_argument("--steps", type=int, default=500)
ap.add_argument("--generations", type=int, default=2000)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--keep", type=float, default=0.5)
a = ap.parse_args()
MIN_S, MAX_S = 3.0, 0.1
H = W = N = 512
P, E = 32, 8


def emit(row):
    print(json.dumps(row), flush=True)
    return row


def noise_problem():
    target = np.random.default_rng(0).uniform(0, 255, (H + 9, W + 5, 3)).astype(np.float32)
    t = prepare_target(target, H, W)
    return t, compute_importance_mask(t, H, W, smooth=3, strength=0.7)


def structured_problem(seed=4):
    """The render of a hidden random genome, mixed half and half with a diagonal gradient."""
    hidden = ga.new_population(1, 96, H, W, 6.0, 0.15, np.random.default_rng(seed))
    img = ggs.render(hidden, H, W, layout="axes")[0]
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    grad = np.stack([xx / (W - 1), yy / (H - 1), 1.0 - (xx + yy) / (H + W - 2)], -1).astype(np.float32)
    t = np.ascontiguousarray(0.5 * img + 0.5 * grad, np.float32)
    return t, compute_importance_mask(t, H, W, smooth=3, strength=0.7)


def events(names):
    out = {}
    for n in names:
        ms, k = api.profile_read(n)
        out[n] = {"ms": ms, "launches": k}
    return out


def cost():
    t, m = structured_problem()
    for K in (1, 8):
        tgt = np.ascontiguousarray(np.repeat(t[None], K, 0))
        wts = np.ascontiguousarray(np.repeat(m[None], K, 0))
        G = ga.new_population(K, N, H, W, MIN_S, MAX_S, np.random.default_rng(5))
        img = ggs.render(G, H, W, layout="axes")
        for c in S.CELLS:
            p = S.SeedParams(c, N, 0, 0.0, 1.5, 200.0)
            for rep in range(3 + a.reps):
                if rep == 3:
                    api.profile_reset()
                    api.profile_enable(True)
                api.seed_sites(G, img, tgt, p, weights=wts, group=1)
            api.profile_enable(False)
            ms, n = api.profile_read("seed")
            emit({"metric": "one placement (cell, rank, apply), HIP events", "K": K, "cell": c,
                  "cells": (-(-H // c)) * (-(-W // c)), "max_sites": N, "calls": n, "us_per_call": 1e3 * ms / max(n, 1)})
        rounds = S.seed_schedule(N, H, W, min_scale_splats=MIN_S, max_scale_splats=MAX_S)
        wall = []
        for rep in range(2 + a.reps):
            if rep == 2:
                api.profile_reset()
                api.profile_enable(True)
            t0 = time.perf_counter()
            ggs.seed_genomes(tgt, N, rounds, weights=wts, min_scale_splats=MIN_S, max_scale_splats=MAX_S)
            if rep >= 2:
                wall.append(time.perf_counter() - t0)
        api.profile_enable(False)
        ev = events(("seed", "prep", "raster"))
        emit({"metric": "one full seeding, default schedule, HIP events", "K": K, "N": N,
              "rounds": [list(r) for r in rounds], "seedings": a.reps,
              "us_placements_per_seeding": 1e3 * ev["seed"]["ms"] / a.reps,
              "us_renders_per_seeding": 1e3 * (ev["prep"]["ms"] + ev["raster"]["ms"]) / a.reps,
              "host_wall_ms_median": 1e3 * float(np.median(wall))})
        for rep in range(3 + a.reps):
            if rep == 3:
                api.profile_reset()
                api.profile_enable(True)
            ggs.render(G, H, W, layout="axes")
        api.profile_enable(False)
        ev = events(("prep", "raster"))
        emit({"metric": "one render call (prep + raster), HIP events", "K": K, "N": N,
              "us_per_call": 1e3 * (ev["prep"]["ms"] + ev["raster"]["ms"]) / a.reps})
        s = DeviceRefine(tgt, wts, G, lr=DEFAULT_LR, min_scale_splats=MIN_S, max_scale_splats=MAX_S, group=1)
        s.run(10)
        s.read()
        t0 = time.perf_counter()
        s.run(a.steps)
        s.read()
        sec = time.perf_counter() - t0
        s.close()
        emit({"metric": "one refine step, host clock", "K": K, "N": N, "steps": a.steps,
              "us_per_step": 1e6 * sec / a.steps})


def refine_best(t, m, G):
    s = DeviceRefine(t, m, G, lr=DEFAULT_LR, min_scale_splats=MIN_S, max_scale_splats=MAX_S)
    try:
        s.run(a.steps)
        return float(s.read()["best_fits"][0])
    finally:
        s.close()


def ga_best(t, m, init, seed):
    cfg = dict(mut_sigma_max={"xy": 0.1, "alog": 0.5, "blog": 0.5, "theta": 0.3, "rgb": 25.0, "alpha": 25.0},
               mut_sigma_min={"xy": 0.01, "alog": 0.05, "blog": 0.05, "theta": 0.025, "rgb": 2.0, "alpha": 2.0},
               schedule="cosine")
    d = DeviceGA(t, m, init, tour_k=2, elite_k=E, cxpb=0.05, mutpb=0.05, min_scale_splats=MIN_S,
                 max_scale_splats=MAX_S, seed=seed, **cfg)
    try:
        d.run(1, a.generations, a.generations)
        return float(d.read()["best_fit"])
    finally:
        d.close()


def effect():
    rows = []
    for name, (t, m) in (("structured", structured_problem()), ("noise", noise_problem())):
        g, placed = ggs.seed_genomes(t, N, weights=m, min_scale_splats=MIN_S, max_scale_splats=MAX_S)
        emit({"target": name, "placed_per_round": placed[:, 0].tolist(),
              "schedule": [list(r) for r in S.seed_schedule(N, H, W, min_scale_splats=MIN_S, max_scale_splats=MAX_S)]})
        fit = lambda pop: ggs.fitness(pop, t, H, W, 3.0, weight_mask=m)  # noqa: E731
        empty = float(fit(S.empty_genome(N, np.log(np.float32(MIN_S)), 1))[0])
        for seed in a.seeds:
            pops = {"seeded": S.seeded_population(P, g[0], H, W, np.random.default_rng(seed), keep=a.keep,
                                                  min_scale_splats=MIN_S, max_scale_splats=MAX_S),
                    "random": ga.new_population(P, N, H, W, MIN_S, MAX_S, np.random.default_rng(seed))}
            for start, pop in pops.items():
                f0 = fit(pop)
                rows.append(emit({"target": name, "seed": seed, "start": start, "empty_canvas": empty,
                                  "start_best": float(f0.min()), "start_mean": float(f0.mean()),
                                  "refine_steps": a.steps, "after_refine": refine_best(t, m, pop[:1]),
                                  "ga_generations": a.generations, "after_ga": ga_best(t, m, pop, seed)}))
    summary = {}
    for name in ("structured", "noise"):
        for start in ("seeded", "random"):
            sel = [r for r in rows if r["target"] == name and r["start"] == start]
            summary[f"{name} {start}"] = {k: {"mean": float(np.mean([r[k] for r in sel])),
                                              "min": float(np.min([r[k] for r in sel])),
                                              "max": float(np.max([r[k] for r in sel]))}
                                          for k in ("start_best", "after_refine", "after_ga")}
    emit({"metric": "fitness (lower is better): mean, min, max over seeds", "seeds": a.seeds, "summary": summary,
          "config": {"H": H, "W": W, "splats": N, "P": P, "keep": a.keep, "refine_steps": a.steps,
                     "ga_generations": a.generations}})


def sweep():
    lo, hi = ga.scale_log_bounds(H, W, MIN_S, MAX_S)
    base = S.seed_schedule(N, H, W, min_scale_splats=MIN_S, max_scale_splats=MAX_S)
    finer = [r._replace(cell=r.cell // 2) for r in base]
    for name, (t, m) in (("structured", structured_problem()), ("noise", noise_problem())):
        fit = lambda pop: ggs.fitness(pop, t, H, W, 3.0, weight_mask=m)  # noqa: E731
        rand = fit(ga.new_population(P, N, H, W, MIN_S, MAX_S, np.random.default_rng(1)))
        emit({"target": name, "random_population_best": float(rand.min()), "random_population_mean": float(rand.mean())})
        for label, rounds in (("default cells", base), ("one size finer", finer)):
            for d in (0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 4.0):
                for alpha in (128.0, 200.0, 255.0):
                    rs = [r._replace(log_sigma=float(np.clip(np.log(np.float32(r.cell / d)), lo, hi)), alpha=alpha)
                          for r in rounds]
                    g, placed = ggs.seed_genomes(t, N, rs, weights=m, min_scale_splats=MIN_S, max_scale_splats=MAX_S)
                    emit({"target": name, "cells": [r.cell for r in rs], "sigma": f"cell / {d:g}", "alpha": alpha,
                          "placed": int(placed.sum()), "seeded_fitness": float(fit(g)[0])})


cost() if a.cost else sweep() if a.sweep else effect()
