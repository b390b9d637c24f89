"""Time of createNewMapPoints' geometry: ydorb_triangulate_matches at 300 and 1500 matches per keyframe pair and 1, 10 (one keyframe's
neighbours as independent problems) and 64 pairs per call, against the test restatement (tests/triangulate_ref/triangulate_ref.cpp, one
CPU thread) on the same batches in the same run.  Both sides are timed at the C entry point on a prebuilt YdTriBatch: median
host-to-host wall time of the synchronous call after warm-up (index checks, the host gather, one upload, the kernel, one read-back),
[min, max] of the repetitions (50 GPU calls, 10 CPU calls) beside it.  Before timing, and again on a cleared output after it, the two
sides' outputs are compared bit for bit.  Prints one JSON line.
--resident times LocalMapping::createNewMapPoints for a whole keyframe instead, at 1000 and 2000 features per
keyframe and 10 and 20 neighbours over about 100 vocabulary nodes: the flat adapter-shaped loop (per neighbour one
ydorb_search_for_triangulation and one ydorb_triangulate_matches call, the map-point flags carried on the host) against ONE
ydorb_mapdb_create_new_points call on a resident table, the two forms alternating within the session, median host-to-host wall time
[min, max] of 15 repetitions each after warm-up.  Before timing the two forms' results are compared exactly.  Per case also: the bytes
each form uploads (computed from the shapes; the resident records' sizes are those of mapdb_tri_kernels.hip.h), the launch counts, and
the device time of the join and gather, of the resolve launches and of the geometry launches from a separate run with the matcher's
profiling on (an event after every launch).  Prints one JSON line."""
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


def resident():
    import mapdb_tri_support as T
    import ydorbslam_amd as y
    from ydorbslam_amd.triangulate import triangulate_matches
    L = lib()
    out = {"metric": "create_new_map_points_ms_per_keyframe", "cases": {}}
    for n in (1000, 2000):
        for nn in (10, 20):
            poses = [S.pose()] + [S.pose(S.rot((0.1 * (k % 3), 1, 0.05), np.radians(3.0 - 0.3 * k)), (0.42 * np.cos(0.6 * k), 0.42 * np.sin(0.6 * k), 0.01 * k))
                                  for k in range(nn)]
            sc = T.Scene(seed=n + nn, n=n, n_nb=nn, nodes=lambda point, kf: (point % 97).astype(np.uint32) * 3 + 1, poses=poses, seen=0.3)
            db, m = y.MapDb(0, 256, 32, 1024), y.OrbMatcher(0.6, False)
            sc.load(db)
            first, nbs, _keep = sc.call()
            A, v1 = sc.kfs[0], sc.kfs[0]["view"]
            fvs = [y.FeatureVector(*k["fv"]) for k in sc.kfs]
            geo = [(T.f12(v1, k["view"]), T.epipole(v1, k["view"])) for k in sc.kfs[1:]]
            has = [(k["row"] >= 0).astype(np.uint8) for k in sc.kfs]

            def flat():
                has0 = has[0].copy()
                res = []
                for i, B in enumerate(sc.kfs[1:]):
                    v2 = B["view"]
                    _, match = m.search_for_triangulation(v1["kps"], A["desc"], has0, v1["right_x"], fvs[0], v2["kps"], B["desc"], has[i + 1], v2["right_x"],
                                                          fvs[i + 1], geo[i][0], geo[i][1], v2["scale_factors"], v2["level_sigma2"])
                    i1 = np.flatnonzero(match >= 0).astype(np.int32)
                    r = triangulate_matches([v1, v2], [dict(first=0, second=1, idx1=i1, idx2=match[i1])])[0] if len(i1) else dict(x3d=np.zeros((0, 3), np.float32), status=np.zeros(0, np.uint8))
                    has0[i1[(r["status"] & 15) == 0]] = 1
                    res.append((i1, match[i1], r["x3d"], r["status"]))
                return res

            def batched():
                return db.create_new_points(m, first, nbs)
            f, b = flat(), batched()
            assert not b["neighbour_status"].any()
            for i, (i1, i2, x, st) in enumerate(f):      # the two forms agree exactly before anything is timed
                assert np.array_equal(np.flatnonzero(b["matched_second"][i] >= 0), i1) and np.array_equal(b["matched_second"][i, i1], i2)
                assert np.array_equal(b["status"][i, i1], st) and np.array_equal(b["x3d"][i, i1].view(np.uint32), x.view(np.uint32))
            for _ in range(3):
                flat(); batched()
            tf, tb = [], []
            for _ in range(15):                          # alternating within the session
                t0 = time.perf_counter(); flat(); t1 = time.perf_counter(); batched(); t2 = time.perf_counter()
                tf.append(t1 - t0); tb.append(t2 - t1)
            L.ydorb_matcher_set_profiling(m._h, 1)
            for _ in range(10):
                batched()
            ms, calls = (C.c_float * 3)(), C.c_int32(0)
            L.ydorb_matcher_create_points_times(m._h, ms, C.byref(calls))
            L.ydorb_matcher_set_profiling(m._h, 0)
            n_feat = [len(k["row"]) for k in sc.kfs]
            matches = [len(i1) for i1, _, _, _ in f]
            nq_flat = [int(np.isin(A["bow"][:, 0], k["bow"][:, 0]).sum()) for k in sc.kfs[1:]]   # an upper bound: the flat join leaves out features with a map point
            up_flat = sum(32 * (n_feat[0] + nk) + 28 * (n_feat[0] + nk) + 4 * nk + nk + n_feat[0] + nk + 16 * q + 48 * mt
                          for nk, q, mt in zip(n_feat[1:], nq_flat, matches))
            up_res = 216 + nn * (384 + 168) + 4 * sum(n_feat)
            stat = lambda ts: [round(float(np.median(ts)) * 1e3, 4), round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]
            out["cases"]["N%d_NB%d" % (n, nn)] = {
                "matches": int(sum(matches)), "accepted": int(b["n_accepted"].sum()), "flat_ms": stat(tf), "resident_ms": stat(tb),
                "flat_upload_bytes_at_most": int(up_flat), "resident_upload_bytes": int(up_res), "flat_launches": 3 * nn, "resident_launches": 2 + 2 * nn,
                "resident_gpu_ms": {"join_gather": round(ms[0], 4), "resolve_chain": round(ms[1], 4), "geometry_chain": round(ms[2], 4), "calls": calls.value}}
            m.close()
            db.close()
    print(json.dumps(out))


if __name__ == "__main__":
    resident() if "--resident" in sys.argv[1:] else main()
