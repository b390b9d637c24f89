"""Throughput of the relocalisation EPnP RANSAC: ydorb_pnp_ransac problems/s at N in {50, 300, 1000} matches and batch in {1, 8, 64}
problems per call, against the test oracle (tests/pnp_ref/pnp_ref.cpp, one CPU thread) on the same problems in the same run.
Workload: 60 % outliers and minInliers above N's reach, so nothing returns and all 300 hypotheses run (the first iterate(5) of a
candidate under ORB-SLAM2's ||).  GPU time = median wall time of the synchronous call after warm-up (packing, one upload, the kernels,
one read-back); prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pnp_support import ref_ransac, synth_problem  # noqa: E402
from ydorbslam_amd import pnp  # noqa: E402


def median_time(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    out = {"metric": "pnp_problems_per_s", "ransac": {}}
    for N in (50, 300, 1000):
        ps = []
        for k in range(64):
            p = synth_problem(N, 10 * N + k, outliers=0.6, max_its=300, n_hyp=300)[0]
            p["min_inliers"] = N   # count >= N needs every match an inlier: with 60 % outliers nothing qualifies
            ps.append(p)
        cpu = median_time(lambda: [ref_ransac(p, 5) for p in ps[:4]], 3) / 4
        for B in (1, 8, 64):
            pnp.ransac(ps[:B])   # warm-up: scratch allocation, code-object load
            g = median_time(lambda: pnp.ransac(ps[:B]), 10)
            out["ransac"]["N%d_B%d" % (N, B)] = {"gpu_problems_per_s": round(B / g, 1), "cpu_problems_per_s": round(1 / cpu, 1),
                                                 "gpu_ms_per_call": round(g * 1e3, 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
