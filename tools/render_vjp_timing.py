"""The render VJP beside the fitness gradient, and a torch optimiser through
ggs.autograd.render_splats (docs/EXPERIMENTS.md §27).  Nothing here is a pass/fail bar.

  (a) device time of one ggs_render_vjp_device call against one
      ggs_fitness_grad_device call (and the forward ggs_fitness_device call for
      scale) at 512 x 512 / 256 splats, B = 32 and B = 128, weighted mode: HIP events
      on the launch stream around --calls calls after --warmup calls, the three
      entry points alternated inside each of --reps repetitions; median and range
      over the repetitions;
  (b) --adam-steps torch.optim.Adam steps on an L1 loss through render_splats
      (layout "axes"), starting from the best individual of the shipped GA shape
      (512 x 512, 512 splats, pop 32, elite 8) after --generations generations on
      tools/de_quality.py's seeded noise target: steps/s (host clock around a
      synchronised loop) and the loss before and after.  The per-column step sizes
      are ggs.refine.DEFAULT_LR, starting values, not tuned.

Prints one JSON line per measurement.

usage: python tools/render_vjp_timing.py [--reps 7] [--calls 10] [--adam-steps 200]"""
import argparse, json, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "genetic-gaussian-splats_amd"))
import ggs
from ggs import api, ga, hip
from ggs.ga_device import DeviceGAIslands
from ggs.mask import compute_importance_mask, prepare_target
from ggs.refine import DEFAULT_LR

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--batches", type=int, nargs="+", default=[32, 128])
ap.add_argument("--generations", type=int, default=20000)
ap.add_argument("--adam-steps", type=int, default=200)
a = ap.parse_args()
H = W = 512
target = np.random.default_rng(0).uniform(0, 255, (H + 9, W + 5, 3)).astype(np.float32)
t = prepare_target(target, H, W)
m = compute_importance_mask(t, H, W, smooth=3, strength=0.7)


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def time_calls(N, B):
    G = ga.new_population(B, N, H, W, 3.0, 0.1, np.random.default_rng(B))
    G = np.ascontiguousarray(np.stack(G), np.float32)
    V = np.random.default_rng(1).standard_normal((B, H, W, 3)).astype(np.float32)
    g, v, dt, dm = (hip.DeviceArray.from_host(x) for x in (G, V, t, m))
    grad, fit = hip.DeviceArray((B, N, 9)), hip.DeviceArray((B,))
    st = hip.Stream()
    calls = {
        "render_vjp": lambda: api.render_vjp_device(0, st.handle, g.ptr, B, N, 9, ggs.GGS_LAYOUT_AXES, H, W, 3.0,
                                                    v.ptr, grad.ptr),
        "fitness_grad": lambda: api.fitness_grad_device(0, st.handle, g.ptr, B, N, 9, dt.ptr, dm.ptr,
                                                        ggs.GGS_FIT_WEIGHTED, 1.0, H, W, 3.0, fit.ptr, grad.ptr),
        "fitness": lambda: api.fitness_device(0, st.handle, g.ptr, B, N, 9, dt.ptr, dm.ptr, ggs.GGS_FIT_WEIGHTED, 1.0,
                                              H, W, 3.0, fit.ptr),
    }
    ms = {k: [] for k in calls}
    for f in calls.values():
        for _ in range(a.warmup):
            f()
    st.synchronize()
    e0, e1 = hip.Event(), hip.Event()
    for _ in range(a.reps):
        for k, f in calls.items():
            e0.record(st)
            for _ in range(a.calls):
                f()
            e1.record(st)
            st.synchronize()
            ms[k].append(e0.elapsed_ms(e1) / a.calls)
    row = {"metric": "device ms per call (HIP events on the launch stream)", "H": H, "W": W, "splats": N, "B": B,
           "reps": a.reps, "calls_per_rep": a.calls, "warmup_calls": a.warmup}
    row.update({k: stats(x) for k, x in ms.items()})
    row["vjp_over_fitness_grad"] = row["render_vjp"]["median_ms"] / row["fitness_grad"]["median_ms"]
    print(json.dumps(row), flush=True)


for B in a.batches:
    time_calls(256, B)

if a.adam_steps > 0:
    import torch
    from ggs.autograd import render_splats
    N, P = 512, 32
    cfg = dict(mut_sigma_max={"xy": 0.1, "alog": 0.5, "blog": 0.5, "theta": 0.3, "rgb": 25.0, "alpha": 25.0},
               mut_sigma_min={"xy": 0.01, "alog": 0.05, "blog": 0.05, "theta": 0.025, "rgb": 2.0, "alpha": 2.0},
               schedule="cosine")
    pop = np.stack([ga.new_population(P, N, H, W, 3.0, 0.1, np.random.default_rng(1))])
    grp = DeviceGAIslands(t, m, pop, [1], 0, 0, tour_k=2, elite_k=8, cxpb=0.05, mutpb=0.05, min_scale_splats=3.0,
                          max_scale_splats=0.1, **cfg)
    try:
        grp.run(1, a.generations, a.generations)
        state = grp.read()
    finally:
        grp.close()
    best = np.ascontiguousarray(np.asarray(state["best"], np.float32).reshape(-1, N, 9)[:1])
    g0 = torch.tensor(best, device="cuda")
    tt = torch.tensor(t, device="cuda")
    lr = torch.tensor(list(DEFAULT_LR), device="cuda", dtype=torch.float32)
    z = torch.zeros_like(g0, requires_grad=True)          # g0 + lr * z: one rate per column through one optimiser
    opt = torch.optim.Adam([z], lr=1.0)

    def l1():
        return (render_splats(g0 + lr * z, H, W, layout="axes") - tt).abs().mean()

    for _ in range(3):                                     # warm-up: allocations, code objects (no optimiser step)
        l1().backward()
        opt.zero_grad()
    start = float(l1().detach())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.adam_steps):
        opt.zero_grad()
        loss = l1()
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    print(json.dumps({"metric": "torch.optim.Adam on an L1 loss through render_splats", "H": H, "W": W, "splats": N,
                      "B": 1, "ga_generations": a.generations, "ga_best_fitness": float(np.min(state["best_fit"])),
                      "adam_steps": a.adam_steps, "steps_per_s": a.adam_steps / sec, "l1_start": start,
                      "l1_final": float(l1().detach()), "lr": list(map(float, DEFAULT_LR)),
                      "timing": "host clock around a synchronised loop"}), flush=True)
