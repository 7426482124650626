"""Density control of the refiner measured: what it costs and what it does.

  --cost    refine steps/s at the shipped shape (512x512, 512 splats), B = 1 and 32, on the
            fitness session (weighted mode) and the loss session: density control off, on
            but never due (the accumulate kernel only) and, with --parent LIB, the parent
            build's library loaded beside this one and alternated in this process.  Host
            clock around run(--steps) + a synchronising read, --reps repetitions after a
            warm-up.  Then the device time of one event (rank, apply, reset) from the
            library's own HIP events (ggs_profile_read("density")) with every = 1, at
            N = 512 on 512x512 and N = 4096 on 256x256.
  (default) plain refine against refine with density control on tools/de_quality.py's seeded
            noise target, from the device GA's best (--generations) and from a fresh
            new_population row, for every x alpha_dead of a small grid: at equal steps, and
            at equal wall time (the step count scaled by the two measured rates).
Prints one JSON line per measurement and a summary line.

usage: python tools/density_quality.py [--cost [--parent LIB]] [--seeds 1 2 3] [--steps N]"""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "genetic-gaussian-splats_amd"))
import ggs
from ggs import _lib, api, ga
from ggs.ga_device import DeviceGA, DeviceRefine, _config
from ggs.mask import compute_importance_mask, prepare_target
from ggs.refine import DEFAULT_LR, DensityParams

ap = argparse.ArgumentParser()
ap.add_argument("--cost", action="store_true")
ap.add_argument("--parent", default=None)
ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
ap.add_argument("--steps", type=int, default=None)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--generations", type=int, default=20000)
ap.add_argument("--every", type=int, nargs="+", default=[50, 200])
ap.add_argument("--alpha-dead", type=float, nargs="+", default=[2.0, 8.0])
ap.add_argument("--grad-min", type=float, default=DensityParams().grad_min)
a = ap.parse_args()
MIN_S, MAX_S = 3.0, 0.1
LOSS = ggs.LossParams(0.8, 0.0, 0.2)
_f32p = C.POINTER(C.c_float)


def problem(H, W):
    target = np.random.default_rng(0).uniform(0, 255, (H + 9, W + 5, 3)).astype(np.float32)
    t = prepare_target(target, H, W)
    return t, compute_importance_mask(t, H, W, smooth=3, strength=0.7)


def emit(row):
    print(json.dumps(row), flush=True)
    return row


class RawRefine:
    """A refine session of any libggs build through ctypes alone (run / sync only)."""

    def __init__(self, lib, t, m, G, loss):
        B, N, _ = G.shape
        H, W = t.shape[:2]
        zero = dict.fromkeys(("xy", "alog", "blog", "theta", "rgb", "alpha"), 0.0)
        cfg = _config(B, N, H, W, 1, 0, 0.0, 0.0, 3.0, MIN_S, MAX_S, None if loss else m, False, 1.0, "linear", zero,
                      zero, 0)
        prm = _lib.RefineParams((C.c_float * 9)(*DEFAULT_LR), 0.9, 0.999, 1e-8)
        self.lib, self.h = lib, C.c_void_p()
        G = np.ascontiguousarray(G, np.float32)
        if loss:
            lp = api.loss_params_c(LOSS)
            rc = lib.ggs_refine_create_loss(0, C.byref(cfg), C.byref(prm), C.byref(lp), None, t.ctypes.data_as(_f32p),
                                            1, G.ctypes.data_as(_f32p), B, B, C.byref(self.h))
        else:
            rc = lib.ggs_refine_create(0, C.byref(cfg), C.byref(prm), t.ctypes.data_as(_f32p), m.ctypes.data_as(_f32p),
                                       G.ctypes.data_as(_f32p), B, C.byref(self.h))
        assert rc == 0, (rc, lib.ggs_last_error())
        self.fits = np.empty(B, np.float32)

    def set_density(self, p):
        prm = ggs.refine.density_params_c(p)
        assert self.lib.ggs_refine_set_density(self.h, C.byref(prm)) == 0

    def timed(self, steps):
        t0 = time.perf_counter()
        assert self.lib.ggs_refine_run(self.h, steps) == 0
        assert self.lib.ggs_refine_read(self.h, None, self.fits.ctypes.data_as(_f32p), None, None, None) == 0
        return time.perf_counter() - t0

    def close(self):
        self.lib.ggs_refine_destroy(self.h)


def load_other(path):
    lib = C.CDLL(os.path.abspath(path))
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    assert not hasattr(lib, "ggs_refine_set_density"), "--parent must be the parent build"
    return lib


def cost():
    import ggs.refine  # noqa: F401
    H = W = N = 512
    t, m = problem(H, W)
    steps = a.steps or 200
    never = DensityParams(every=10 ** 9, start=0)
    libs = {"off": _lib.lib, "never_due": _lib.lib}
    if a.parent:
        libs = {"parent": load_other(a.parent), **libs}
    for loss in (False, True):
        for B in (1, 32):
            G = ga.new_population(B, N, H, W, MIN_S, MAX_S, np.random.default_rng(5))
            rates = {k: [] for k in libs}
            for rep in range(a.reps + 1):                     # the first pass warms up and is dropped
                for k, lib in libs.items():
                    s = RawRefine(lib, t, m, G, loss)
                    if k == "never_due":
                        s.set_density(never)
                    s.timed(10)
                    sec = s.timed(steps)
                    s.close()
                    if rep:
                        rates[k].append(steps / sec)
            emit({"metric": "refine steps/s", "session": "loss" if loss else "fitness", "B": B, "steps": steps,
                  **{k: {"median": float(np.median(v)), "runs": [round(x, 1) for x in v]} for k, v in rates.items()}})
    for (H, W, N, B) in ((512, 512, 512, 1), (512, 512, 512, 32), (256, 256, 4096, 1), (256, 256, 4096, 8)):
        t, m = problem(H, W)
        G = ga.new_population(B, N, H, W, MIN_S, MAX_S, np.random.default_rng(6))
        s = DeviceRefine(t, m, G, lr=DEFAULT_LR, min_scale_splats=MIN_S, max_scale_splats=MAX_S)
        # new_population's alphas lie in [180, 255]: about half the splats start dead, every
        # live one is a source, and the rank kernel has the same work whatever moves
        s.set_density(DensityParams(every=1, start=0, max_moves=N, alpha_dead=220.0, grad_min=0.0))
        s.run(5)
        s.read()
        api.profile_reset()
        api.profile_enable(True)
        s.run(40)
        st = s.density_stats()
        api.profile_enable(False)
        ms, n = api.profile_read("density")
        s.close()
        emit({"metric": "one density event (rank, apply, reset), HIP events", "H": H, "W": W, "N": N, "B": B,
              "events": n, "us_per_event": 1e3 * ms / max(n, 1), "pairs_moved_in_45_events": int(st["moves"].sum())})


def refine_run(t, m, G, steps, density):
    s = DeviceRefine(t, m, G, lr=DEFAULT_LR, min_scale_splats=MIN_S, max_scale_splats=MAX_S)
    try:
        if density is not None:
            s.set_density(density)
        t0 = time.perf_counter()
        s.run(steps)
        r = s.read()
        sec = time.perf_counter() - t0
        moved = int(s.density_stats()["moves"].sum()) if density is not None else 0
        splits = int(s.density_stats()["splits"].sum()) if density is not None else 0
        return float(r["best_fits"][0]), float(r["fitness"][0]), sec, moved, splits
    finally:
        s.close()


def effect():
    H = W = N = 512
    P, E = 32, 8
    t, m = problem(H, W)
    steps = a.steps or 2000
    cfg = dict(mut_sigma_max={"xy": 0.1, "alog": 0.5, "blog": 0.5, "theta": 0.3, "rgb": 25.0, "alpha": 25.0},
               mut_sigma_min={"xy": 0.01, "alog": 0.05, "blog": 0.05, "theta": 0.025, "rgb": 2.0, "alpha": 2.0},
               schedule="cosine")
    grid = [(e, ad) for e in a.every for ad in a.alpha_dead]
    refine_run(t, m, ga.new_population(1, N, H, W, MIN_S, MAX_S, np.random.default_rng(0)), 50, None)   # warm-up
    rows = []
    for seed in a.seeds:
        init = ga.new_population(P, N, H, W, MIN_S, MAX_S, np.random.default_rng(seed))
        dga = DeviceGA(t, m, init, tour_k=2, elite_k=E, cxpb=0.05, mutpb=0.05, min_scale_splats=MIN_S,
                       max_scale_splats=MAX_S, seed=seed, **cfg)
        dga.run(1, a.generations, a.generations)
        st = dga.read()
        dga.close()
        starts = {"ga_best": np.ascontiguousarray(st["best"], np.float32).reshape(1, N, 9), "fresh": init[:1]}
        for name, G in starts.items():
            dead0 = {ad: int((G[0, :, 8] < ad).sum()) for ad in a.alpha_dead}
            best, last, sec, _, _ = refine_run(t, m, G, steps, None)
            rows.append(emit({"seed": seed, "start": name, "run": "plain", "steps": steps, "best": best, "last": last,
                              "wall_s": sec, "dead_at_start": dead0}))
            for e, ad in grid:
                d = DensityParams(every=e, start=e, alpha_dead=ad, grad_min=a.grad_min)
                b1, l1, s1, mv, sp = refine_run(t, m, G, steps, d)
                rows.append(emit({"seed": seed, "start": name, "run": "density", "at": "equal steps", "every": e,
                                  "alpha_dead": ad, "steps": steps, "best": b1, "last": l1, "wall_s": s1,
                                  "moved": mv, "splits": sp}))
                n2 = max(int(steps * sec / s1), 1)             # the steps that fit the plain run's wall time
                b2, l2, s2, mv, sp = refine_run(t, m, G, n2, d)
                rows.append(emit({"seed": seed, "start": name, "run": "density", "at": "equal wall", "every": e,
                                  "alpha_dead": ad, "steps": n2, "best": b2, "last": l2, "wall_s": s2, "moved": mv,
                                  "splits": sp}))
    summary = {}
    for name in ("ga_best", "fresh"):
        sel = [r for r in rows if r["start"] == name]
        summary[name] = {"plain": float(np.mean([r["best"] for r in sel if r["run"] == "plain"]))}
        for e, ad in grid:
            for at in ("equal steps", "equal wall"):
                v = [r["best"] for r in sel if r["run"] == "density" and (r["every"], r["alpha_dead"], r["at"]) == (e, ad, at)]
                summary[name][f"every={e} alpha_dead={ad} {at}"] = float(np.mean(v))
    emit({"metric": "best fitness, mean over seeds", "steps": steps, "ga_generations": a.generations,
          "summary": summary, "config": {"H": H, "W": W, "splats": N, "grad_min": a.grad_min, "defaults": DensityParams()._asdict()}})


cost() if a.cost else effect()
