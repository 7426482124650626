"""Per-wave clocks of the raster under the bench's stream schedule (diagnostic build
GGS_TIMING=1, see wave_timing.py): are the wave slots full with several rasters in
flight, and do the waves themselves run slower than with one?

    make -C genetic-gaussian-splats_amd/csrc probe PROBE=-DGGS_TIMING=1
    GGS_PROBE=1 GGS_LIB=genetic-gaussian-splats_amd/libggs_probe.so \
        python tools/probe/wave_timing_streams.py --streams 4

Enqueues --steps batches of the bench workload (512^2 / 256 splats / B = 128,
weighted fitness, one plan) round-robin over --streams streams, as bench.py does,
times them on the host, and reads g_ggs_timing.  Every launch writes the same
16,384 slots (one per blockIdx), so what is read is, per slot, the last launch
that wrote it: a sample of 16,384 waves from the end of the run.  Per wave:
realtime duration (100 MHz counter), s_memtime ticks over the same span, visits.
From the host time per step and the mean wave duration:
    mean live waves = waves per launch * mean wave duration / time per step
(Little's law; 3,072 = every slot of 256 CUs x 4 SIMDs x 3 waves taken).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "genetic-gaussian-splats_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4)
    ap.add_argument("--steps", type=int, default=2000)
    a = ap.parse_args()
    os.environ.setdefault("GGS_HIP_RUNTIME", "system")
    if int(os.environ.get("GPU_MAX_HW_QUEUES", "4") or 4) < 8:      # as bench.py
        os.environ["GPU_MAX_HW_QUEUES"] = "8"
    import bench
    import ggs
    from ggs import hip
    H = W = 512
    N, B = 256, 128
    ggs.ensure_init()
    hip.set_device(0)
    rng = np.random.default_rng(1234)
    pops = [hip.DeviceArray.from_host(bench.synthetic_population(B, N, i)) for i in range(4)]
    tgt = hip.DeviceArray.from_host(rng.uniform(0, 1, (H, W, 3)).astype(np.float32))
    mask = hip.DeviceArray.from_host(rng.uniform(0.405, 1, (H, W)).astype(np.float32))
    outs = [hip.DeviceArray((B,)) for _ in range(8)]
    streams = [hip.Stream() for _ in range(a.streams)]
    plan = ggs.TargetPlan(0, streams[0].handle, tgt.ptr, mask.ptr, ggs.GGS_FIT_WEIGHTED, 1.0, H, W)
    streams[0].synchronize()

    def run(n):
        for i in range(n):
            plan.fitness_device(streams[i % a.streams].handle, pops[i % 4].ptr, B, N, 9, 3.0, outs[i % 8].ptr)
        for s in streams:
            s.synchronize()

    run(a.steps)                                    # clock ramp
    t0 = time.perf_counter()
    run(a.steps)
    us_step = (time.perf_counter() - t0) / a.steps * 1e6
    n_waves = B * 32 * 4
    buf = np.zeros((n_waves, 8), np.uint64)
    fn = ggs.lib.ggs_debug_timing_read
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_size_t]
    assert fn(buf.ctypes.data, buf.nbytes) == 0, "ggs_debug_timing_read failed (not a GGS_TIMING build?)"
    dur = (buf[:, 1].astype(np.int64) - buf[:, 0].astype(np.int64)) / 100.0          # us
    ticks = buf[:, 2].astype(np.float64) + buf[:, 3].astype(np.float64) + buf[:, 4].astype(np.float64)
    vis = buf[:, 3].astype(np.float64)
    visits = buf[:, 6].astype(np.float64)
    ok = (dur > 0) & (dur < 1e4)                    # a slot two launches wrote at once is dropped
    print(json.dumps({
        "streams": a.streams, "steps": a.steps, "us_per_step": us_step, "waves_sampled": int(ok.sum()),
        "wave_us": {"mean": float(dur[ok].mean()), "p50": float(np.median(dur[ok])),
                    "p99": float(np.percentile(dur[ok], 99))},
        "mean_live_waves": float(n_waves * dur[ok].mean() / us_step),
        "memtime_ticks_per_us": float(ticks[ok].sum() / dur[ok].sum()),
        "ticks_per_visit": float(vis[ok].sum() / max(visits[ok].sum(), 1)),
        "us_per_visit": float((vis[ok] / np.maximum(ticks[ok], 1) * dur[ok]).sum() / max(visits[ok].sum(), 1)),
        "phase_frac": {"cull": float(buf[ok, 2].astype(np.float64).sum() / ticks[ok].sum()),
                       "visits": float(vis[ok].sum() / ticks[ok].sum()),
                       "epilogue": float(buf[ok, 4].astype(np.float64).sum() / ticks[ok].sum())}}))
    plan.close()


if __name__ == "__main__":
    main()
