"""Throughput of the loop-closure Sim3 check: ydorb_sim3_ransac and ydorb_sim3_optimize problems/s at N in {50, 300, 1000} pairs and batch
in {1, 8, 64} problems per call, against the test oracle (tests/sim3_ref/sim3_ref.cpp, one CPU thread) on the same problems in the same run.
RANSAC workload: 60 % outliers and minInliers = N, so no hypothesis returns and all 300 of setRansacParameters' cap are evaluated (the
worst case of one candidate).  optimizeSim3 workload: 10 % gross outliers, both stages run.  GPU time = median wall time of the synchronous
call after warm-up (packing, one upload, the kernels, one read-back); prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from sim3_support import ref_optimize, ref_ransac, synth_optimize, synth_ransac  # noqa: E402
from ydorbslam_amd import sim3  # noqa: E402


def median_time(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    out = {"metric": "sim3_problems_per_s", "ransac": {}, "optimize": {}}
    for N in (50, 300, 1000):
        rp = [synth_ransac(N, 10 * N + k, fix_scale=bool(k % 2), outliers=0.6, min_inliers=N, max_its=300)[0] for k in range(64)]
        op = [synth_optimize(N, 10 * N + k, fix_scale=bool(k % 2), outliers=0.1) for k in range(64)]
        cpu_r = median_time(lambda: [ref_ransac(p, 5) for p in rp[:8]], 3) / 8
        cpu_o = median_time(lambda: [ref_optimize(p) for p in op[:8]], 3) / 8
        for B in (1, 8, 64):
            sim3.ransac(rp[:B]); sim3.optimize_sim3(op[:B])   # warm-up: scratch allocation, code-object load
            g_r = median_time(lambda: sim3.ransac(rp[:B]), 20)
            g_o = median_time(lambda: sim3.optimize_sim3(op[:B]), 20)
            key = "N%d_B%d" % (N, B)
            out["ransac"][key] = {"gpu_problems_per_s": round(B / g_r, 1), "cpu_problems_per_s": round(1 / cpu_r, 1),
                                  "gpu_ms_per_call": round(g_r * 1e3, 3)}
            out["optimize"][key] = {"gpu_problems_per_s": round(B / g_o, 1), "cpu_problems_per_s": round(1 / cpu_o, 1),
                                    "gpu_ms_per_call": round(g_o * 1e3, 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
