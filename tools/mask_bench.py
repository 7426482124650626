"""Target preparation + importance mask for K images: the host numpy path
(ggs.mask, image by image) against the device path (csrc/ggs_mask.hip) on the same
machine (docs/EXPERIMENTS.md §20).

Per shape, after --warmup unmeasured calls, the median of --repeats:
  host_ms      wall time of prepare_targets(backend="host")
  device_ms    wall time of prepare_targets(backend="device"): upload, kernels,
               download, ending in the library's stream synchronise
  kernels_ms   device time of ggs_targets_prepare_device on inputs resident in HBM,
               from HIP events around the enqueue on one stream
and max|device - host| of the masks and targets the timed calls produced.
Shapes: K = 8 640x480 -> 512^2 (a batch of frames) and K = 1 2048^2 (the SA
configuration's canvas); 8-bit-range inputs, the reference's mask arguments.

--fixtures adds one line with max|device - host| of the mask (and target) for every
reference fixture under tests/golden/ that tests/test_gpu_mask.py checks.

usage: python tools/mask_bench.py [--repeats 5] [--warmup 2] [--shapes frames,big] [--fixtures]
One JSON line per shape.  Fails without a GPU."""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "genetic-gaussian-splats_amd"))
import ggs
from ggs import _lib, hip
from ggs import mask as gm

SHAPES = {"frames": (8, 480, 640, 512, 512), "big": (1, 2048, 2048, 2048, 2048)}
KW = dict(edge_scales=(1, 2, 4), w_edge=0.7, w_var=0.3, gamma=0.7, floor=0.15, smooth=3, strength=0.7)

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--shapes", default="frames,big")
ap.add_argument("--fixtures", action="store_true")
a = ap.parse_args()
assert ggs.ensure_init() >= 1, "no HIP device"
hip.set_device(0)


def wall(fn, warmup):
    for _ in range(warmup):
        out = fn()
    ts = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return ts, out


def textured(rng, h, w):
    """Low-frequency structure under noise (the conditioning of a photograph, not of white noise)."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = 0.5 + 0.3 * np.sin(xx / rng.uniform(20, 60)) * np.cos(yy / rng.uniform(20, 60))
    img = base[..., None] * rng.uniform(0.6, 1.0, 3).astype(np.float32) + rng.uniform(-0.15, 0.15, (h, w, 3))
    return np.round(np.clip(img, 0, 1) * 255).astype(np.float32)


def fixture_diffs():
    gold = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
    mk, fit = np.load(os.path.join(gold, "mask.npz")), np.load(os.path.join(gold, "fitness.npz"))
    h512, edges = np.load(os.path.join(gold, "headline_512.npz")), np.load(os.path.join(gold, "mask_edges.npz"))
    cases = [("mask.npz 96x80 s1.0", mk["target"], 96, 80, 1.0), ("mask.npz 96x80 s0.7", mk["target"], 96, 80, 0.7),
             ("mask.npz 100x70->64x48", mk["target_u8"], 64, 48, 0.7),
             ("mask.npz 100x70->150x90", mk["target_u8"], 150, 90, 0.7)]
    cases += [(f"fitness.npz {c}", fit[f"{c}__target"], *(int(v) for v in fit[f"{c}__HW"]), 0.7)
              for c in ("f64", "f128", "f40x56")]
    cases += [("headline_512.npz", h512["target_u8"], 512, 512, 0.7)]
    cases += [(f"mask_edges.npz {c}", edges[f"{c}__image"], *(int(v) for v in edges[f"{c}__HW"]),
               float(edges[f"{c}__strength"]))
              for c in ("t33x47", "t9x13", "u8_100x70", "max400", "stack0", "stack1", "stack2")]
    out = {}
    for name, img, H, W, strength in cases:
        kw = {**KW, "strength": strength}
        ht, hm = gm.prepare_targets([img], H, W, backend="host", **kw)
        dt, dm = gm.prepare_targets([img], H, W, backend="device", device=0, **kw)
        out[name] = {"mask": float(np.abs(dm - hm).max()), "target": float(np.abs(dt - ht).max())}
    print(json.dumps({"max_abs_device_minus_host": out}), flush=True)


if a.fixtures:
    fixture_diffs()
for name in [s for s in a.shapes.split(",") if s]:
    K, H0, W0, H, W = SHAPES[name]
    rng = np.random.default_rng(19)
    imgs = np.stack([textured(rng, H0, W0) for _ in range(K)])
    host_ts, (ht, hm) = wall(lambda: gm.prepare_targets(imgs, H, W, backend="host", **KW), min(a.warmup, 1))
    dev_ts, (dt, dm) = wall(lambda: gm.prepare_targets(imgs, H, W, backend="device", device=0, **KW), a.warmup)

    st = hip.Stream()
    d_img = hip.DeviceArray.from_host(imgs)
    d_t, d_m = hip.DeviceArray((K, H, W, 3)), hip.DeviceArray((K, H, W))
    prm = gm.mask_params(**KW)
    e0, e1 = hip.Event(), hip.Event()

    def kernels():
        e0.record(st)
        _lib.check(ggs.lib.ggs_targets_prepare_device(0, C.c_void_p(st.handle), C.c_void_p(d_img.ptr), K, H0, W0,
                                                      H, W, prm, C.c_void_p(d_t.ptr), C.c_void_p(d_m.ptr)),
                   "ggs_targets_prepare_device")
        e1.record(st)
        return e0.elapsed_ms(e1)

    for _ in range(a.warmup):
        kernels()
    k_ts = [kernels() for _ in range(a.repeats)]
    same = bool(np.array_equal(d_m.to_host(st), dm) and np.array_equal(d_t.to_host(st), dt))
    for x in (d_img, d_t, d_m):
        x.free()
    print(json.dumps({"shape": name, "K": K, "in": [H0, W0], "work": [H, W],
                      "host_ms": round(float(np.median(host_ts)), 2),
                      "device_ms": round(float(np.median(dev_ts)), 2),
                      "kernels_ms": round(float(np.median(k_ts)), 3),
                      "host_over_device": round(float(np.median(host_ts) / np.median(dev_ts)), 1),
                      "repeats": {"host_ms": [round(t, 1) for t in host_ts], "device_ms": [round(t, 2) for t in dev_ts],
                                  "kernels_ms": [round(t, 3) for t in k_ts]},
                      "max_abs_mask_diff": float(np.abs(dm - hm).max()),
                      "max_abs_target_diff": float(np.abs(dt - ht).max()),
                      "device_form_equals_host_form": same,
                      "lib": os.path.basename(ggs.LIB_PATH)}), flush=True)
