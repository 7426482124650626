"""Raster counters of a tools/profile_streams.sh PMC run: per-dispatch means over
the last --steps raster dispatches and VALU busy by the project's rule
(SQ_ACTIVE_INST_VALU * 4 / (GRBM_GUI_ACTIVE / 8 * 1024), tools/round_profile.sh)."""
import argparse, collections, csv, glob, json, os

ap = argparse.ArgumentParser()
ap.add_argument("root")
ap.add_argument("--steps", type=int, default=200)
a = ap.parse_args()
by = collections.defaultdict(dict)
for f in glob.glob(os.path.join(a.root, "**", "*counter_collection.csv"), recursive=True):
    for r in csv.DictReader(open(f)):
        if "raster_kernel" in r["Kernel_Name"]:
            by[int(r["Dispatch_Id"])][r["Counter_Name"]] = float(r["Counter_Value"])
rows = [by[k] for k in sorted(by)][-a.steps:]
mean = {c: sum(r[c] for r in rows) / len(rows) for c in rows[0]}
busy = [r["SQ_ACTIVE_INST_VALU"] * 4 / (r["GRBM_GUI_ACTIVE"] / 8 * 1024) for r in rows]
print(json.dumps({"dispatches": len(rows), "counters": mean,
                  "valu_busy": {"mean": sum(busy) / len(busy), "min": min(busy), "max": max(busy)},
                  "note": "counter collection serialises dispatches: each raster runs alone"}, indent=1))
