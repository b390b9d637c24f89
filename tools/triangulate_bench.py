"""Time of createNewMapPoints' geometry: ydorb_triangulate_matches at 300 and 1500 matches per keyframe pair and 1, 10 (one keyframe's
neighbours as independent problems) and 64 pairs per call, against the test restatement (tests/triangulate_ref/triangulate_ref.cpp, one
CPU thread) on the same batches in the same run.  Both sides are timed at the C entry point on a prebuilt YdTriBatch: median
host-to-host wall time of the synchronous call after warm-up (index checks, the host gather, one upload, the kernel, one read-back),
[min, max] of the repetitions (50 GPU calls, 10 CPU calls) beside it.  Before timing, and again on a cleared output after it, the two
sides' outputs are compared bit for bit.  Prints one JSON line."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import triangulate_support as S  # noqa: E402
from ydorbslam_amd import lib  # noqa: E402
from ydorbslam_amd.triangulate import TriBatch  # noqa: E402


def pair_views(m, seed):
    """Two keyframes 0.45 m apart seeing m points: mixed mono / stereo, 0.7 px noise, octave mismatches."""
    rng = np.random.default_rng(seed)
    T = [S.pose(), S.pose(S.rot((0.1, 1, 0.05), np.radians(4.0)), (0.45, 0.03, 0.05))]
    vb = [S.ViewBuilder(t) for t in T]
    z = rng.uniform(1.0, 12.0, m)
    X = np.stack([rng.uniform(-0.4, 0.4, m) * z, rng.uniform(-0.3, 0.3, m) * z, z], axis=1)
    for k in range(m):
        o = int(rng.integers(0, 8))
        for v in range(2):
            uv, d = S.project(T[v], X[k:k + 1])
            vb[v].add(uv[0] + rng.normal(0, 0.7, 2), o if v == 0 or rng.uniform() > 0.15 else (o + 4) % 8, d[0] if rng.uniform() < 0.5 else None,
                      rng.normal(0, 0.7))
    return [v.view() for v in vb]


def times(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    L, R = lib(), S.ref()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    out = {"metric": "triangulate_matches_per_s", "cases": {}}
    for m in (300, 1500):
        views = pair_views(m, m)
        rng = np.random.default_rng(m)
        for nb in (1, 10, 64):
            probs = []
            for _ in range(nb):
                i1 = rng.permutation(m).astype(np.int32)
                i2 = i1.copy()
                wrong = rng.uniform(size=m) < 0.2
                i2[wrong] = rng.integers(0, m, int(wrong.sum()))
                probs.append(dict(first=0, second=1, idx1=i1, idx2=i2))
            B = TriBatch(views, probs)
            x, st, na = B.outputs()
            xr, sr, nr = B.outputs()
            gpu = lambda: L.ydorb_triangulate_matches(C.byref(B.struct), p(x), p(st), p(na))
            cpu = lambda: R.triref_triangulate(C.byref(B.struct), p(xr), p(sr), p(nr))
            if gpu() != 0:
                raise SystemExit("ydorb_triangulate_matches failed: " + L.ydorb_last_error().decode())
            cpu()
            assert np.array_equal(st, sr) and np.array_equal(x.view(np.uint32), xr.view(np.uint32)) and np.array_equal(na, nr)
            for _ in range(5):
                gpu()
            g, c = times(gpu, 50), times(cpu, 10)
            x[:], st[:], na[:] = 0, 0, 0
            assert gpu() == 0 and np.array_equal(st, sr) and np.array_equal(x.view(np.uint32), xr.view(np.uint32)) and np.array_equal(na, nr)
            out["cases"]["M%d_B%d" % (m, nb)] = {
                "accepted": int(na.sum()), "matches": B.M,
                "gpu_ms_per_call": [round(v * 1e3, 4) for v in g], "cpu_ms_per_call": [round(v * 1e3, 4) for v in c],
                "gpu_matches_per_s": round(B.M / g[0]), "cpu_matches_per_s": round(B.M / c[0])}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
