"""The image loss beside the render VJP, and refine sessions on it (docs/EXPERIMENTS.md §29).
Nothing here is a pass/fail bar.

  (a) device time of one call at 512 x 512 / 256 splats, B = 32 and B = 128:
      ggs_image_loss_device with and without a cotangent (the image a device render of
      the genomes, weights 0.8 L1 + 0.2 (1 - SSIM), and L1 alone for scale), beside
      ggs_render_layout_device, ggs_render_vjp_device and the whole ggs_loss_grad_device.
      HIP events on the launch stream around --calls calls after --warmup calls, the entry
      points alternated inside each of --reps repetitions; median and range.
  (b) refine steps/s at the shipped shape (512 x 512, 512 splats), B = 1 and 32, host clock
      around run(n) + a synchronising read after a warm-up run: DeviceRefine(loss=) against
      the MSE refiner (weighted mode, the session of §25) in the same process;
  (c) the same loss written in torch (float32 conv2d, zero padding) over
      ggs.autograd.render_splats with torch.optim.Adam, B = 1 (the loop of §27 with SSIM
      added), and that loop with ggs.autograd.image_loss in place of the torch loss.

Prints one JSON line per measurement.

usage: python tools/loss_timing.py [--reps 7] [--calls 10] [--steps 200]"""
import argparse, json, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "genetic-gaussian-splats_amd"))
import ggs
from ggs import api, ga, hip
from ggs.ga_device import DeviceRefine
from ggs.mask import compute_importance_mask, prepare_target
from ggs.refine import DEFAULT_LR

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--batches", type=int, nargs="+", default=[32, 128])
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--no-torch", action="store_true")
a = ap.parse_args()
H = W = 512
target = np.random.default_rng(0).uniform(0, 255, (H + 9, W + 5, 3)).astype(np.float32)
t = prepare_target(target, H, W)
m = compute_importance_mask(t, H, W, smooth=3, strength=0.7)
LOSS = ggs.LossParams(0.8, 0.0, 0.2)
L1 = ggs.LossParams(1.0, 0.0, 0.0)


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def population(B, N, seed):
    return np.ascontiguousarray(np.stack(ga.new_population(B, N, H, W, 3.0, 0.1, np.random.default_rng(seed))),
                                np.float32)


def time_calls(N, B):
    G = population(B, N, B)
    g, dt = hip.DeviceArray.from_host(G), hip.DeviceArray.from_host(t[None])
    img, cot = hip.DeviceArray((B, H, W, 3)), hip.DeviceArray((B, H, W, 3))
    grad, loss = hip.DeviceArray((B, N, 9)), hip.DeviceArray((B,))
    st = hip.Stream()
    AX = ggs.GGS_LAYOUT_AXES
    calls = {
        "render": lambda: api.render_layout_device(0, st.handle, g.ptr, B, N, 9, AX, H, W, 3.0, img.ptr),
        "image_loss_cot": lambda: api.image_loss_device(0, st.handle, img.ptr, B, dt.ptr, 1, B, H, W, LOSS, loss.ptr,
                                                        cot.ptr),
        "image_loss": lambda: api.image_loss_device(0, st.handle, img.ptr, B, dt.ptr, 1, B, H, W, LOSS, loss.ptr, 0),
        "image_loss_cot_l1_only": lambda: api.image_loss_device(0, st.handle, img.ptr, B, dt.ptr, 1, B, H, W, L1,
                                                                loss.ptr, cot.ptr),
        "render_vjp": lambda: api.render_vjp_device(0, st.handle, g.ptr, B, N, 9, AX, H, W, 3.0, cot.ptr, grad.ptr),
        "loss_grad": lambda: api.loss_grad_device(0, st.handle, g.ptr, B, N, 9, AX, dt.ptr, 1, B, H, W, 3.0, LOSS,
                                                  loss.ptr, grad.ptr),
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
           "reps": a.reps, "calls_per_rep": a.calls, "warmup_calls": a.warmup, "weights": list(LOSS)}
    row.update({k: stats(x) for k, x in ms.items()})
    print(json.dumps(row), flush=True)


def refine_rate(B, N, loss):
    G = population(B, N, 100 + B)
    kw = dict(lr=DEFAULT_LR, min_scale_splats=3.0, max_scale_splats=0.1)
    s = DeviceRefine(t, None, G, loss=loss, **kw) if loss is not None else DeviceRefine(t, m, G, **kw)
    try:
        s.run(10)
        first = s.read()["best_fits"].copy()
        rates = []
        for _ in range(3):
            t0 = time.perf_counter()
            s.run(a.steps)
            r = s.read()
            rates.append(a.steps / (time.perf_counter() - t0))
    finally:
        s.close()
    print(json.dumps({"metric": "refine steps/s (host clock around run + synchronising read)", "H": H, "W": W,
                      "splats": N, "B": B, "loss": None if loss is None else list(loss),
                      "objective": "image loss" if loss is not None else "weighted MSE fitness",
                      "steps_per_run": a.steps, "steps_per_s": statistics.median(rates), "min": min(rates),
                      "max": max(rates), "best_first": float(first[0]), "best_last": float(r["best_fits"][0])}),
          flush=True)


for B in a.batches:
    time_calls(256, B)
for B in (1, 32):
    refine_rate(B, 512, LOSS)
    refine_rate(B, 512, None)

if not a.no_torch:
    import torch
    import torch.nn.functional as F
    from ggs.autograd import image_loss, render_splats
    N = 512
    g0 = torch.tensor(population(1, N, 101), device="cuda")
    tt = torch.tensor(t, device="cuda")
    lr = torch.tensor(list(DEFAULT_LR), device="cuda", dtype=torch.float32)
    i = torch.arange(11, dtype=torch.float64) - 5
    g1 = torch.exp(-(i * i) / 4.5)
    g1 = (g1 / g1.sum()).to(torch.float32)
    win = (g1[:, None] * g1[None, :])[None, None].expand(3, 1, -1, -1).contiguous().cuda()
    yc = tt.permute(2, 0, 1)[None]
    C1, C2 = 0.01 ** 2, 0.03 ** 2

    def conv(z):
        return F.conv2d(z, win, padding=5, groups=3)

    def torch_loss(img):
        xc = img.permute(0, 3, 1, 2)
        mux, muy = conv(xc), conv(yc)
        sxx, syy, sxy = conv(xc * xc) - mux * mux, conv(yc * yc) - muy * muy, conv(xc * yc) - mux * muy
        ssim = ((2 * mux * muy + C1) * (2 * sxy + C2)) / ((mux * mux + muy * muy + C1) * (sxx + syy + C2))
        return 0.8 * (img - tt).abs().mean() + 0.2 * (1.0 - ssim.mean())

    def library_loss(img):
        return image_loss(img, tt, LOSS).sum()

    for name, fn in (("torch-written L1 + SSIM (float32)", torch_loss), ("ggs.autograd.image_loss", library_loss)):
        z = torch.zeros_like(g0, requires_grad=True)          # g0 + lr * z: one rate per column through one optimiser
        opt = torch.optim.Adam([z], lr=1.0)

        def value():
            return fn(render_splats(g0 + lr * z, H, W, layout="axes"))

        for _ in range(3):                                     # warm-up: allocations, code objects (no optimiser step)
            value().backward()
            opt.zero_grad()
        start = float(value().detach())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            opt.zero_grad()
            loss = value()
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        print(json.dumps({"metric": "torch.optim.Adam through render_splats", "loss": name, "H": H, "W": W,
                          "splats": N, "B": 1, "steps": a.steps, "steps_per_s": a.steps / sec, "loss_start": start,
                          "loss_final": float(value().detach()), "timing": "host clock around a synchronised loop"}),
              flush=True)
