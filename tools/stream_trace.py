"""Summarise a rocprofv3 kernel trace of the bench's multi-stream pass
(tools/profile_streams.sh): for prep, raster and finalize, over the last --steps
steps of the run (the timed pass),
  queue delay   start minus the end of the previous kernel on the same stream
                (prep's predecessor is the previous step's finalize, so its delay
                also holds any wait for the host's enqueue; raster and finalize
                follow a kernel enqueued back to back with them),
  duration,
  rasters       how many raster dispatches of other streams overlap it,
and for the pass the share of time with 0, 1, 2, ... rasters in flight.  A kernel
trace has no per-workgroup times, so "no raster has undispatched workgroups" is
bounded, not measured: it holds at least while no raster is in flight
(rasters_in_flight["0"]).

    python3 tools/stream_trace.py <dir with *kernel_trace.csv> [--steps 200]
"""
import argparse, collections, csv, glob, json, os, statistics


def classify(name):
    for k in ("prep_kernel", "raster_kernel", "raster_multi_kernel", "finalize_kernel"):
        if k in name:
            return k.replace("_kernel", "").replace("raster_multi", "raster")
    return None


def q(v, p):
    v = sorted(v)
    return v[min(len(v) - 1, int(p * len(v)))] if v else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("root")
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    ev = []
    for f in glob.glob(os.path.join(a.root, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            c = classify(r["Kernel_Name"])
            if c:
                ev.append({"c": c, "s": int(r["Start_Timestamp"]), "e": int(r["End_Timestamp"]),
                           "q": r.get("Stream_Id") or r.get("Queue_Id"), "wg": r.get("Workgroup_Size")})
    ev.sort(key=lambda x: x["s"])
    by_q = collections.defaultdict(list)
    for x in ev:
        by_q[x["q"]].append(x)
    for lst in by_q.values():
        for prev, x in zip(lst, lst[1:]):
            x["delay"] = (x["s"] - prev["e"]) / 1e3
    ras_all = [x for x in ev if x["c"] == "raster"]
    ras = ras_all[-a.steps:]
    t0 = ras[0]["s"]
    # the pass: from just before its first raster to the finalize of its last one
    # (bench.py --full launches a few prep kernels of its own long after the pass)
    t_last = max(x["e"] for x in ras)
    win = [x for x in ev if t0 - 50_000 <= x["s"] <= t_last + 50_000]
    t1 = max(x["e"] for x in win)
    out = {"steps": len(ras), "streams": len({x["q"] for x in win}), "pass_us": (t1 - t0) / 1e3,
           "us_per_step": (t1 - t0) / 1e3 / len(ras), "kernels": {}}
    for c in ("prep", "raster", "finalize"):
        xs = [x for x in win if x["c"] == c]
        if not xs:
            continue
        dl = [x["delay"] for x in xs if "delay" in x]
        du = [(x["e"] - x["s"]) / 1e3 for x in xs]
        ov = [sum(1 for r in ras_all if r["q"] != x["q"] and r["s"] < x["e"] and r["e"] > x["s"]) for x in xs]
        ov_start = [sum(1 for r in ras_all if r["q"] != x["q"] and r["s"] < x["s"] < r["e"]) for x in xs]
        out["kernels"][c] = {
            "n": len(xs), "workgroup": xs[-1]["wg"],
            "queue_delay_us": {"median": statistics.median(dl), "p10": q(dl, 0.1), "p90": q(dl, 0.9),
                               "mean": statistics.fmean(dl)},
            "duration_us": {"median": statistics.median(du), "p10": q(du, 0.1), "p90": q(du, 0.9),
                            "mean": statistics.fmean(du)},
            "rasters_overlapping_mean": statistics.fmean(ov),
            "rasters_running_at_start_mean": statistics.fmean(ov_start)}
    # rasters in flight over the pass
    edges = []
    for r in ras_all:
        if r["e"] > t0 and r["s"] < t1:
            edges += [(max(r["s"], t0), 1), (min(r["e"], t1), -1)]
    edges.sort()
    share, n, last = collections.Counter(), 0, t0
    for t, d in edges:
        share[n] += t - last
        n, last = n + d, t
    share[n] += t1 - last
    out["rasters_in_flight"] = {str(k): round(v / (t1 - t0), 4) for k, v in sorted(share.items())}
    out["raster_busy_sum_over_pass"] = round(sum(min(r["e"], t1) - max(r["s"], t0) for r in ras_all
                                                 if r["e"] > t0 and r["s"] < t1) / (t1 - t0), 4)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
