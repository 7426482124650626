"""SA chain groups: chain-iterations/s of K annealing chains in one session
(ggs_sa_chains_*) against K sessions in a row, on the device loop's defaults
(adaptive width, cosine temperature from --temp0, --tries tries per iteration).

--mode shared   one DeviceSAChains group, all chains on one target
--mode targets  one DeviceSAChains group, a target per chain
--mode solo     K DeviceSA sessions one after the other on the same inputs: a target
                each, or with --one-target all on target 0, the pair of `shared` (also
                runs on an older library: GGS_LIB=libggs_<rev>.so)
--chains 1 compares a single-chain group (shared) with a lone session (solo).

Each session anneals --warm + --iters iterations of one schedule: the first --warm
are not timed (--warm 0 measures the start of a run, where most tries are
accepted; a few hundred put the timed part late in the run, where acceptances are
rare and rounds are wide), then --iters iterations are timed, ending in the run's
own device sync; --repeats times in one process, one JSON line with every repeat.
The chains' seeds, initial individuals and targets are the same in every mode, so
chain k follows the same trajectory in all three.

usage: python tools/bench_sa_chains.py --mode shared [--chains 8] [--size 512] [--splats 256]
                                       [--tries 8] [--iters 200] [--warm 0] [--repeats 3]"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "genetic-gaussian-splats_amd"))
import ggs
from ggs import annealing as A
from ggs import ga
from ggs.ga_device import DeviceSA
from ggs.mask import compute_importance_mask, prepare_target

ap = argparse.ArgumentParser()
ap.add_argument("--mode", required=True, choices=["shared", "targets", "solo"])
ap.add_argument("--chains", type=int, default=8)
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--splats", type=int, default=256)
ap.add_argument("--tries", type=int, default=8)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--warm", type=int, default=0)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--mutpb", type=float, default=0.05)
ap.add_argument("--temp0", type=float, default=1e-3)
ap.add_argument("--one-target", action="store_true", help="solo: every session on target 0 (the pair of shared)")
ap.add_argument("--width", type=int, default=0, help="fixed round width (0: adaptive, the default)")
a = ap.parse_args()
K, H, W, n, w0 = a.chains, a.size, a.size, a.iters, a.warm
total = w0 + n
cfg = dict(mut_sigma_max={"xy": 0.1, "alog": 0.5, "blog": 0.5, "theta": 0.3, "rgb": 25.0, "alpha": 25.0},
           mut_sigma_min={"xy": 0.01, "alog": 0.05, "blog": 0.05, "theta": 0.025, "rgb": 2.0, "alpha": 2.0},
           schedule="cosine", mutpb=a.mutpb, min_scale_splats=3.0, max_scale_splats=0.1,
           max_tries=A.device_loop_width(H, W, a.tries))
per_chain = a.mode == "targets" or (a.mode == "solo" and not a.one_target)
nt = K if per_chain else 1
t = np.stack([prepare_target(np.random.default_rng(k).uniform(0, 255, (H, W, 3)).astype(np.float32), H, W)
              for k in range(nt)])
m = np.stack([compute_importance_mask(x, H, W, smooth=3, strength=0.7) for x in t]).astype(np.float32)
init = np.stack([ga.new_population(1, a.splats, H, W, 3.0, 0.1, np.random.default_rng(100 + k))[0]
                 for k in range(K)])
seeds = [1 + k for k in range(K)]
temps = np.asarray([A.temp_schedule("cosine", a.temp0, i, total) for i in range(total)], np.float64)


def timed(session, tt):
    """(seconds of the timed part, the session's loop state) — warm part first, untimed."""
    if w0:
        session.run(0, tt[..., :w0], total, a.tries, a.width)
    else:                                             # first launches of the process / session
        session.run(0, tt[..., :1], total, a.tries, a.width)
    first = max(w0, 1)
    t0 = time.perf_counter()
    session.run(first, tt[..., first:], total, a.tries, a.width)
    return time.perf_counter() - t0, session.loop_state()


its = total - max(w0, 1)                              # timed iterations per chain
times, stats = [], None
for _ in range(a.repeats):
    if a.mode == "solo":
        dt, rounds, ev, acc, best = 0.0, 0, 0, 0, []
        for k in range(K):
            kt = k if per_chain and nt > 1 else 0
            s = DeviceSA(t[kt], m[kt], init[k], seed=seeds[k], **cfg)
            try:
                d, st = timed(s, temps)
                dt += d
                rounds += st["rounds"]
                ev += st["evaluated"]
                acc += st["accepted"]
                best.append(st["best_fit"])
            finally:
                s.close()
        stats = {"rounds": rounds, "evaluated": ev, "accepted": acc, "best_fit": best}
    else:
        from ggs.ga_device import DeviceSAChains
        s = DeviceSAChains(t if per_chain else t[0], m if per_chain else m[0], init, seeds, **cfg)
        try:
            dt, st = timed(s, np.repeat(temps[None], K, axis=0))
        finally:
            s.close()
        stats = {"rounds": int(st["rounds"].max()), "evaluated": int(st["evaluated"].sum()),
                 "accepted": int(st["accepted"].sum()), "best_fit": st["best_fit"].tolist()}
    times.append(dt)
rates = [K * its / d for d in times]
med = float(np.median(times))
print(json.dumps({"metric": "chain-iterations/s", "mode": a.mode, "lib": os.path.basename(ggs.LIB_PATH),
                  "value": round(float(np.median(rates)), 1), "repeats": [round(r, 1) for r in rates],
                  "ms_per_group_iteration": round(1e3 * med / its, 4),
                  "config": {"H": H, "W": W, "splats": a.splats, "chains": K, "tries": a.tries, "iters": n,
                             "warm": w0, "temp0": a.temp0, "width": a.width, "cap": cfg["max_tries"]},
                  # counters over the whole session (warm part included)
                  **stats}))
