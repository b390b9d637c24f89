"""Time of one essential-graph optimisation (ydorb_essential_graph_optimize) on ring graphs with covisibility chords and one loop, at 100,
500 and 1500 keyframes, beside the test restatement (tests/essgraph_ref/essgraph_ref.cpp, one CPU thread) on the same graph in the same run.
GPU figure: wall time of the synchronous call, host to host (list building, one upload, every LM trial with its read-back, the map-point
correction, one read-back): median and [min, max] after a warm-up call.  A second pass with the event pairs on
(ydorb_essential_graph_set_profiling) splits the device time into linearize / assemble / factorise + solve / update / trial chi2; its wall
time is not reported, the events slow the host.  Prints one JSON line.  --sizes 100,500 for a shorter run."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import essgraph_support as S  # noqa: E402
from ydorbslam_amd import essential_graph as eg  # noqa: E402


def bench_graph(n, fix_scale=True):
    """Spanning chain i -> i - 1, covisibility chords to i - 2 and (every third keyframe) i - 5, the loop connection (n - 1, 0); vertex 0
    (the loop keyframe) fixed; drift 0.002 per keyframe; 20 map points per keyframe."""
    edges = [(n - 1, 0)] + [(i, i - 1) for i in range(1, n)] + [(i, i - 2) for i in range(2, n)] + [(i, i - 5) for i in range(5, n, 3)]
    g = S.make_graph(n, edges, 1000 + n, fix_scale, drift=0.002, name="ring%d" % n)
    pts, ref = S.map_points(20 * n, n, n)
    return g, pts, ref


def call(g, pts, ref):
    return eg.optimize_essential_graph(g["sim3"], g["fixed"], g["edges"], g["meas"], pts, ref, fix_scale=g["fix_scale"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100,500,1500")
    ap.add_argument("--no-cpu", action="store_true", help="skip the restatement (its dense factor at 1500 keyframes takes 1.8 GB)")
    args = ap.parse_args()
    out = {"metric": "essential_graph_ms_per_call", "sizes": {}}
    for n in [int(v) for v in args.sizes.split(",")]:
        g, pts, ref = bench_graph(n)
        reps = 10 if n <= 100 else 5 if n <= 500 else 3
        r = call(g, pts, ref)   # warm-up: scratch allocation, code-object load
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = call(g, pts, ref)
            ts.append((time.perf_counter() - t0) * 1e3)
        eg.set_profiling(True)
        p = call(g, pts, ref)
        eg.set_profiling(False)
        row = {"edges": len(g["edges"]), "rows": 7 * (n - 1), "iterations": r["n_iterations"], "trials": r["n_trials"],
               "gpu_ms_median": round(float(np.median(ts)), 3), "gpu_ms_min": round(min(ts), 3), "gpu_ms_max": round(max(ts), 3), "reps": reps,
               "device_ms": {k: round(float(v), 3) for k, v in p["ms"].items()},
               "chi2_first_last": [float(r["log_chi2"][0]), float(r["log_chi2"][-1])],
               "distance_to_truth": S.distance(r["sim3"], g["truth"])}
        if not args.no_cpu:
            t0 = time.perf_counter()
            c = S.ref_optimize(g, pts, ref)
            row["cpu_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            row["cpu_trials"] = c["n_trials"]
            row["gpu_to_cpu_distance"] = S.distance(r["sim3"], c["sim3"])
        out["sizes"][str(n)] = row
        eg.release()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
