#!/usr/bin/env python3
"""Global BA on trajectory-shaped maps: the dense reduced camera solve against the block-skyline one.

Workload: ydorbslam_amd.synth.trajectory_ba_problem with one loop closure (every point seen by `span` consecutive keyframes, the last
keyframes tied to the first points, keyframe 0 fixed), solved with the global-BA options.  DENSE and SKYLINE at 200 / 800 / 1 600 /
3 200 free keyframes, SKYLINE alone at 3 300, 6 000 and 20 000.  Time per LM trial is device time from the events YdBaResult carries
(ms_total and the per-phase sums, divided by the trials); the host planning time (pair list, ordering, envelope: ydorb_ba_plan, which
touches no device) is reported beside it.  Every shape is warmed up with one untimed solve; every repetition is a process of its own, and
the table holds the median with the minimum and maximum over the processes.  It reports, it does not gate.

  python tools/global_ba_bench.py [--processes 3] [--iterations 3] [--span 3] [--per-kf 4] [--sizes 200,800,...] [--child]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BOTH = (200, 800, 1600, 3200)
SKYLINE_ONLY = (3300, 6000, 20000)
DENSE, SKYLINE = 1, 2


def shapes(sizes):
    """smallest first, the dense solve of the largest map last (it is the longest step)"""
    out = [(SKYLINE, n) for n in sizes]
    out += [(DENSE, n) for n in sizes if n <= 3200]
    return out


def child(args):
    import numpy as np   # noqa: F401
    import ydorbslam_amd as y
    from ydorbslam_amd.synth import trajectory_ba_problem
    problems = {}
    y.lib()   # loaded before anything is timed
    for solver, n in shapes(args.sizes):
        if n not in problems:
            problems[n] = trajectory_ba_problem(n + 1, span=args.span, per_kf=args.per_kf, loop=True, seed=n, noise_px=1.0)
        prob = problems[n]
        t0 = time.perf_counter()
        info = y.Optimizer.plan(prob, solver=SKYLINE)
        plan_ms = 1e3 * (time.perf_counter() - t0)
        o = y.Optimizer.global_options(args.iterations, True)
        o.flags |= 4   # YDORB_BA_PHASE_TIMES
        y.Optimizer.local_bundle_adjust(prob, o, solver=solver)                 # warm-up: allocations, code objects, clocks
        t0 = time.perf_counter()
        r = y.Optimizer.local_bundle_adjust(prob, o, solver=solver)
        wall_ms = 1e3 * (time.perf_counter() - t0)
        trials = max(r["trials"], 1)
        row = dict(solver="dense" if solver == DENSE else "skyline", n_free=n, trials=r["trials"], wall_ms=wall_ms, plan_ms=plan_ms,
                   ordering=info["ordering_used"], envelope_blocks=info["envelope_blocks"], covisible_pairs=info["covisible_pairs"],
                   chi2=float(r["log"][-1, 0]) if len(r["log"]) else None)
        for k, v in r["ms"].items():
            row["ms_" + k] = float(v) / trials
        print(json.dumps(row), flush=True)
        y.Optimizer.release()


def parent(args):
    runs = {}
    for p in range(args.processes):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--iterations", str(args.iterations), "--span", str(args.span),
               "--per-kf", str(args.per_kf), "--sizes", ",".join(map(str, args.sizes))]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.timeout)
        for line in r.stdout.splitlines():
            if line.startswith("{"):
                row = json.loads(line)
                runs.setdefault((row["solver"], row["n_free"]), []).append(row)
        if r.returncode != 0:
            print("process %d ended with status %d: stopping" % (p, r.returncode), file=sys.stderr)
            break

    def mmm(rows, key):
        v = [row[key] for row in rows]
        return "%.3g (%.3g .. %.3g)" % (statistics.median(v), min(v), max(v))

    print("| free keyframes | solver | ms per trial: total | Schur | solve | host plan, ms | trials | envelope blocks | processes |")
    print("|---|---|---|---|---|---|---|---|---|")
    for (solver, n), rows in sorted(runs.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        print("| %d | %s | %s | %s | %s | %s | %d | %d | %d |" % (n, solver, mmm(rows, "ms_total"), mmm(rows, "ms_schur"), mmm(rows, "ms_solve"),
                                                              mmm(rows, "plan_ms"), rows[0]["trials"], rows[0]["envelope_blocks"], len(rows)))
    print(json.dumps({"global_ba_bench": {"%s-%d" % k: [r["ms_total"] for r in v] for k, v in runs.items()}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--span", type=int, default=3)
    ap.add_argument("--per-kf", type=int, default=4)
    ap.add_argument("--sizes", type=lambda s: tuple(int(v) for v in s.split(",")), default=BOTH + SKYLINE_ONLY)
    ap.add_argument("--timeout", type=float, default=600.0, help="seconds per process")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    (child if args.child else parent)(args)


if __name__ == "__main__":
    main()
