"""Time of one essential-graph optimisation on ring graphs with covisibility chords and one loop, at 100, 500 and 1500 keyframes (--sizes
for others; the dense solver stops at 2 742), beside the test restatement on one CPU thread on the same graph in the same run.
--solver dense (default: ydorb_essential_graph_optimize), skyline, auto, or both: skyline and dense alternating call by call, so that
the two see the same machine state.  --ordering smaller | natural | rcm for the skyline.
GPU figure: wall time of the synchronous call, host to host (list building, the plan, one upload, every LM trial with its read-back, the
map-point correction, one read-back): median and [min, max] after a warm-up call.  A second pass with the event pairs on
(ydorb_essential_graph_set_profiling) splits the device time into linearize / assemble / factorise + solve / update / trial chi2; its wall
time is not reported, the events slow the host.  CPU: the skyline restatement (tests/essgraph_ref/essgraph_skyline_ref.cpp), which
returns the dense one's bytes and holds the envelope only.  Prints one JSON line: per size the graph's figures and the envelope, one
sub-object per solver that ran ("dense", "skyline" or "auto": iterations, trials, gpu_ms_*, device_ms, per-trial figures) and "cpu".
--sizes 100,500 for a shorter run."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import essgraph_skyline_support as K  # noqa: E402
import essgraph_support as S  # noqa: E402
from ydorbslam_amd import essential_graph as eg  # noqa: E402


def bench_graph(n, fix_scale=True):
    """Spanning chain i -> i - 1, covisibility chords to i - 2 and (every third keyframe) i - 5, the loop connection (n - 1, 0); vertex 0
    (the loop keyframe) fixed; drift 0.002 per keyframe; 20 map points per keyframe."""
    g = S.make_graph(n, K.chord_ring_edges(n), 1000 + n, fix_scale, drift=0.002, name="ring%d" % n)
    pts, ref = S.map_points(20 * n, n, n)
    return g, pts, ref


def call(g, pts, ref, solver, ordering):
    kw = {} if solver == "dense" else dict(solver=solver, ordering=ordering)
    return eg.optimize_essential_graph(g["sim3"], g["fixed"], g["edges"], g["meas"], pts, ref, fix_scale=g["fix_scale"], **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100,500,1500")
    ap.add_argument("--solver", default="dense", choices=["dense", "skyline", "auto", "both"])
    ap.add_argument("--ordering", default="smaller", choices=["smaller", "natural", "rcm"])
    ap.add_argument("--no-cpu", action="store_true", help="skip the restatement")
    args = ap.parse_args()
    out = {"metric": "essential_graph_ms_per_call", "solver": args.solver, "ordering": args.ordering, "sizes": {}}
    if not args.no_cpu:
        K.sky_ref()   # compiled here, not inside the first timed call
    for n in [int(v) for v in args.sizes.split(",")]:
        g, pts, ref = bench_graph(n)
        solvers = ["skyline", "dense"] if args.solver == "both" else [args.solver]
        # the dense solver's limit is the library's to state: AUTO plans DENSE exactly while the graph fits it
        fits_dense = eg.plan(g["sim3"], g["fixed"], g["edges"], g["meas"], solver="auto")["solver_used"] == "dense"
        solvers = [s for s in solvers if s != "dense" or fits_dense]
        reps = 10 if n <= 100 else 5 if n <= 500 else 3
        last, ts = {}, {s: [] for s in solvers}
        for s in solvers:
            last[s] = call(g, pts, ref, s, args.ordering)   # warm-up: scratch allocation, code-object load
        for _ in range(reps):
            for s in solvers:   # alternating
                t0 = time.perf_counter()
                last[s] = call(g, pts, ref, s, args.ordering)
                ts[s].append((time.perf_counter() - t0) * 1e3)
        plan = eg.plan(g["sim3"], g["fixed"], g["edges"], g["meas"], solver="skyline", ordering=args.ordering, max_factor_bytes=1 << 62)
        row = {"edges": len(g["edges"]), "rows": 7 * (n - 1), "reps": reps,
               "envelope": {"ordering_used": plan["ordering_used"], "max_row_blocks": plan["max_row_blocks"],
                            "blocks_natural": plan["envelope_blocks_natural"], "bytes_natural": 392 * plan["envelope_blocks_natural"],
                            "blocks_rcm": plan["envelope_blocks_rcm"], "bytes_rcm": 392 * plan["envelope_blocks_rcm"]}}
        eg.set_profiling(True)
        for s in solvers:
            r, p = last[s], call(g, pts, ref, s, args.ordering)
            row[s] = {"iterations": r["n_iterations"], "trials": r["n_trials"], "gpu_ms_median": round(float(np.median(ts[s])), 3),
                      "gpu_ms_min": round(min(ts[s]), 3), "gpu_ms_max": round(max(ts[s]), 3),
                      "device_ms": {k: round(float(v), 3) for k, v in p["ms"].items()},
                      "solve_ms_per_trial": round(float(p["ms"]["solve"]) / p["n_trials"], 4),
                      "gpu_ms_per_trial": round(float(np.median(ts[s])) / r["n_trials"], 4),
                      "chi2_first_last": [float(r["log_chi2"][0]), float(r["log_chi2"][-1])],
                      "distance_to_truth": S.distance(r["sim3"], g["truth"])}
        eg.set_profiling(False)
        if not args.no_cpu:
            t0 = time.perf_counter()
            c = K.sky_ref_optimize(g, pts, ref)
            ms = (time.perf_counter() - t0) * 1e3
            row["cpu"] = {"ms": round(ms, 3), "trials": c["n_trials"], "ms_per_trial": round(ms / c["n_trials"], 4), "skyline_doubles": c["skyline_doubles"]}
            for s in solvers:
                row[s]["gpu_to_cpu_distance"] = S.distance(last[s]["sim3"], c["sim3"])
        out["sizes"][str(n)] = row
        eg.release()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
