"""Time of the graph assembly of localBundleAdjust, host to host at the C entry point: 20 / 50 / 100 local
keyframes with 2 000 / 5 000 / 10 000 local points of about 7 views each (tests/mapdb_lba_support.Scene).  Two forms alternate within
each of 15 repetitions after a warm-up, their results compared exactly before the timing:
  (i)  resident    ydorb_mapdb_local_ba_graph with nothing staged: the call itself, its result left in the handle's pinned memory;
  (ii) restated    the sequential loops on flat arrays (tests/localba_ref, one CPU core), the arrays prepared outside the timing.  It
                   walks arrays, not KeyFrame / MapPoint objects and std::maps under locks: it understates the host walk it stands for.
The Python flat assembly (mapdb_lba_support.dict_graph) is timed three times on its own: it is the form the tests compare with, not a
contender.  Per case also the bytes up and down, launches and synchronisations of the call (ydorb_mapdb_lba_stats), and the time of
the solve the graph is handed to (ydorb_ba_solve_with, solver AUTO) on a scene with a consistent geometry, so that the assembly's share
of one localBundleAdjust is stated.  Prints one JSON line."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mapdb_lba_support as S  # noqa: E402
import ydorbslam_amd as y  # noqa: E402
from ydorbslam_amd._lib import YdLocalBaGraph, lib  # noqa: E402
from ydorbslam_amd.optimizer import Optimizer  # noqa: E402

REPS = 15
CASES = ((20, 2000), (50, 5000), (100, 10000))


def med(v):
    return [round(float(x) * 1e3, 4) for x in (np.median(v), min(v), max(v))]


def case(n_local, n_points):
    n_other = 60
    s = S.Scene(seed=n_local, n_local=n_local, n_other=n_other, n_sparse=0, n_local_points=n_points, n_far_points=n_points // 10,
                local_feats=int(n_points * 2.9 / n_local) + 8, other_feats=int(n_points * 12 / n_other) + 8, max_span=14, big_views=0, late=0)
    poses, camera = S.make_geometric(s)
    db = s.load(y.MapDb(0, s.n_points, s.n_kf, 16 * s.n_points))
    L = lib()
    kf, sig, G = np.ascontiguousarray(s.kf_slots), S.SIGMA, YdLocalBaGraph()
    inp = S.ref_inputs(s.tables())
    got, want = db.local_ba_graph(kf, sig), S.ref_graph(s.tables(), kf)
    S.same_graph(got, want)
    part = dict(resident=[], restated=[], python=[])

    def resident():
        t0 = time.perf_counter()
        rc = L.ydorb_mapdb_local_ba_graph(db._h, S._p(kf), len(kf), S._p(sig), C.byref(G))
        part["resident"].append(time.perf_counter() - t0)
        assert rc == 0

    def restated():
        t0 = time.perf_counter()
        S.ref_run(inp, kf, sig)
        part["restated"].append(time.perf_counter() - t0)

    for _ in range(3):
        resident(); restated()
    for v in part.values():
        v.clear()
    for _ in range(REPS):
        resident(); restated()
    for _ in range(3):
        t0 = time.perf_counter()
        S.dict_graph(s.tables(), kf)
        part["python"].append(time.perf_counter() - t0)
    S.same_graph(db.local_ba_graph(kf, sig), want)
    st = db.lba_stats()
    db.lba_set_profiling(True)                                   # a run of its own: the event pairs cost stream time
    phases = []
    for _ in range(REPS):
        resident()
        ps = db.lba_stats()
        phases.append([ps[k] for k in ("last_ms_points", "last_ms_walk", "last_ms_emit", "last_ms_copy")])
    profiled = part["resident"][-REPS:]
    del part["resident"][-REPS:]
    db.lba_set_profiling(False)
    graph = dict(want, pose_fixed=np.where(want["pose_kf"] == 0, 1, want["pose_fixed"]).astype(np.uint8))
    prob = S.problem_of(graph, poses[graph["pose_kf"]], camera)
    solve = []
    for _ in range(4):                                           # the first solve allocates
        t0 = time.perf_counter()
        r = Optimizer.local_bundle_adjust(prob, solver=0)
        solve.append(time.perf_counter() - t0)
    out = {k + "_ms": med(v) for k, v in part.items()}
    out.update(profiled_resident_ms=med(profiled), gpu_ms=dict(zip(("points", "walk", "emit", "copy"), [round(float(v), 4) for v in np.median(np.array(phases), axis=0)])))
    out.update(solve_ms=med(solve[1:]), solve_trials=int(r["trials"]), n_local=st["last_n_local"], n_fixed=st["last_n_fixed"], n_points=st["last_n_points"],
               n_edges=st["last_n_edges"], upload_bytes=st["last_upload_bytes"], download_bytes=st["last_download_bytes"], launches=st["last_launches"],
               syncs=st["last_syncs"], views_per_point=round(st["last_n_edges"] / max(st["last_n_points"], 1), 2))
    out["assembly_share_of_resident_lba"] = round(out["resident_ms"][0] / (out["resident_ms"][0] + out["solve_ms"][0]), 4)
    out["assembly_share_of_restated_lba"] = round(out["restated_ms"][0] / (out["restated_ms"][0] + out["solve_ms"][0]), 4)
    db.close()
    return out


def main():
    out = {"metric": "local_ba_assembly_ms", "reps": REPS, "cases": {}}
    for n_local, n_points in CASES:
        out["cases"]["kf%d_points%d" % (n_local, n_points)] = case(n_local, n_points)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
