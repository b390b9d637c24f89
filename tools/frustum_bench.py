"""Time of Tracking::searchLocalPoints' numeric part, host to host at the C entry points, for local maps of 1000 / 3000 / 8000 points
against frames of 1000 / 2000 keypoints (tests/frustum_support.local_map scenarios):
  (a) fused        ydorb_search_local_points: one call, the queries are built on the device;
  (b) composition  ydorb_frustum_cull, the query build on the host (numpy, timed on its own), ydorb_search_by_projection;
  (c) host cull    the test restatement (tests/frustum_ref, one CPU thread), the same host query build, ydorb_search_by_projection:
                   what the adapter did before (its query build is a C++ loop, so read (c) without the build column too).
Median wall time of the synchronous calls after warm-up, [min, max] of the repetitions beside it.  A second table times
ydorb_frustum_cull alone at 1, 8 and 64 views of 3000 points over one shared table, against the restatement.  Before and after timing
the outputs of (a), (b) and (c) are compared bit for bit.  Prints one JSON line.
With --resident it times the per-frame local-map step on the resident map table instead, for local maps of
300 / 2000 / 8000 points listed by slot out of a map twice that size:
  (i)   flat       a host gather of the listed points into a YdMapPointTable, then ydorb_search_local_points; the gather is a numpy
                   index over map-wide arrays, timed on its own - the reference's walk over MapPoint pointers is not measured;
  (ii)  resident   ydorb_mapdb_search_local_points with nothing staged;
  (iii) restaged   ydorb_mapdb_set_point_attributes of every listed point, then the same call (the staging timed on its own too).
The three alternate within each repetition; their results are compared exactly before and after.  Bytes uploaded per call are counted
from the arguments (flat) and from the handle's sync counters (resident)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import frustum_support as S  # noqa: E402
import ydorbslam_amd as y  # noqa: E402
from ydorbslam_amd.frustum import TRACK_DTYPE, FrustumBatch  # noqa: E402

TH, RATIO, REPS = 3.0, 0.8, 30
p = lambda a: a.ctypes.data_as(C.c_void_p)


def times(fn, reps=REPS):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return [round(float(v) * 1e3, 4) for v in (np.median(ts), min(ts), max(ts))]


def search_case(L, R, m, n_kp, n_mp):
    s = S.local_map(seed=n_kp + n_mp, n_kp=n_kp, n_mp=n_mp, th=TH)
    frame = y.FrameView(s["kps"], s["desc"], S.BOUNDS, s["right_x"])
    fv, table, view = frame.c(), s["table"], s["view"]
    B = FrustumBatch([view], table, [np.arange(n_mp)], [s["skip"]])
    lg = np.array([s["log"], 0], np.float32)
    sf = S.scale_factors()
    has_obs = s["has_obs"]
    out = {}

    def buffers():
        return dict(rows=np.zeros(n_mp, TRACK_DTYPE), status=np.zeros(n_mp, np.uint8), taken=s["taken"].copy(),
                    assigned=np.full(n_kp, -1, np.int32), n_in=np.zeros(1, np.int32), n_to=C.c_int32(0), n_m=C.c_int32(0))

    a, b, c = buffers(), buffers(), buffers()
    part = {}

    def fused():
        a["taken"][:], a["assigned"][:] = s["taken"], -1
        assert L.ydorb_search_local_points(m._h, C.byref(fv), C.byref(view), C.byref(table.struct), p(s["skip"]), p(has_obs), TH, RATIO, p(a["taken"]),
                                           p(a["assigned"]), p(a["rows"]), p(a["status"]), C.byref(a["n_to"]), C.byref(a["n_m"])) == 0

    def rest(d, cull):
        d["taken"][:], d["assigned"][:] = s["taken"], -1
        t0 = time.perf_counter()
        cull()
        t1 = time.perf_counter()
        q = S.queries_from_rows(d["rows"], d["status"], has_obs, TH, sf)
        t2 = time.perf_counter()
        assert L.ydorb_search_by_projection(m._h, 0, C.byref(fv), p(q), p(table.desc), n_mp, RATIO, 0, 0, p(d["taken"]), p(d["assigned"]), C.byref(d["n_m"])) == 0
        part.setdefault(id(d), []).append((t1 - t0, t2 - t1, time.perf_counter() - t2))

    def composed():
        rest(b, lambda: L.ydorb_frustum_cull(C.byref(B.struct), p(b["rows"]), p(b["status"]), p(b["n_in"])))

    def host_cull():
        rest(c, lambda: R.frustumref_cull(C.byref(B.struct), p(lg), p(c["rows"]), p(c["status"]), p(c["n_in"])))

    def check():
        fused(); composed(); host_cull()
        for d in (b, c):
            assert np.array_equal(a["rows"].tobytes(), d["rows"].tobytes()) and np.array_equal(a["status"], d["status"])
            assert np.array_equal(a["assigned"], d["assigned"]) and np.array_equal(a["taken"], d["taken"]) and a["n_m"].value == d["n_m"].value
        assert a["n_to"].value == int(b["n_in"][0]) == int(c["n_in"][0])

    check()
    for fn in (fused, composed, host_cull):
        for _ in range(5):
            fn()
    part.clear()
    out["fused_ms"], out["composition_ms"], out["host_cull_ms"] = times(fused), times(composed), times(host_cull)
    for name, d in (("composition", b), ("host_cull", c)):
        med = np.median(np.array(part[id(d)]), axis=0) * 1e3
        out[name + "_parts_ms"] = dict(cull=round(float(med[0]), 4), query_build=round(float(med[1]), 4), search=round(float(med[2]), 4))
    for d in (a, b, c):
        d["rows"][:], d["status"][:] = 0, 9
    check()
    out["in_view"], out["matches"] = a["n_to"].value, a["n_m"].value
    return out


def cull_case(L, R, n_views, n_mp=3000):
    s = S.local_map(seed=77, n_kp=500, n_mp=n_mp, th=TH)
    rng = np.random.default_rng(n_views)
    views, logs = [], []
    for f in range(n_views):
        v, lg = S.view(*S.pose(S.rot((0.2, 1, 0.1), np.radians(7.0 + 0.2 * f)), (0.3 + 0.01 * f, -0.1, 0.2)))
        views.append(v); logs.append(lg)
    B = FrustumBatch(views, s["table"], [rng.permutation(n_mp) for _ in range(n_views)], [s["skip"]] * n_views)
    rows, st, n_in = B.outputs()
    rr, sr, nr = B.outputs()
    lg = np.array(logs + [0], np.float32)
    gpu = lambda: L.ydorb_frustum_cull(C.byref(B.struct), p(rows), p(st), p(n_in))
    cpu = lambda: R.frustumref_cull(C.byref(B.struct), p(lg), p(rr), p(sr), p(nr))
    if gpu() != 0:
        raise SystemExit("ydorb_frustum_cull failed: " + L.ydorb_last_error().decode())
    cpu()
    assert rows.tobytes() == rr.tobytes() and np.array_equal(st, sr) and np.array_equal(n_in, nr)
    for _ in range(5):
        gpu()
    g, c = times(gpu, 50), times(cpu, 10)
    rows[:], st[:] = 0, 9
    assert gpu() == 0 and rows.tobytes() == rr.tobytes() and np.array_equal(st, sr)
    return dict(entries=B.L, in_view=int(n_in.sum()), gpu_ms=g, cpu_ms=c)


def resident_case(L, m, n_kp, n_mp):
    s = S.local_map(seed=n_kp + n_mp, n_kp=n_kp, n_mp=n_mp, th=TH)
    frame = y.FrameView(s["kps"], s["desc"], S.BOUNDS, s["right_x"])
    fv, t, view = frame.c(), s["table"], s["view"]
    rng = np.random.default_rng(n_mp)
    universe = 2 * n_mp
    slots = rng.permutation(universe)[:n_mp].astype(np.int32)
    # the map as the host holds it, by slot: what the flat path gathers from
    pos, normal = np.zeros((universe, 3), np.float32), np.zeros((universe, 3), np.float32)
    mn, mx, desc = np.zeros(universe, np.float32), np.zeros(universe, np.float32), np.zeros((universe, 32), np.uint8)
    pos[slots], normal[slots], mx[slots], desc[slots] = t.pos_min[:, :3], t.normal_max[:, :3], t.max_distance, t.desc
    mn[slots] = (t.max_distance / S.scale_factors()[7]).astype(np.float32)
    has_map = np.zeros(universe, np.uint8)
    has_map[slots] = s["has_obs"]
    db = y.MapDb(0, universe, 4, universe)
    db.enable_attributes()
    db.set_centres([0], np.zeros((1, 3), np.float32))
    db.set_points(slots, [np.zeros(1 if h else 0, np.int32) for h in s["has_obs"]], [np.zeros(1 if h else 0, np.uint8) for h in s["has_obs"]],
                  np.zeros(n_mp, np.uint8), np.zeros(n_mp, np.int32), np.zeros(n_mp, np.uint8), pos[slots])
    db.set_point_attributes(slots, normal[slots], mn[slots], mx[slots], desc[slots])
    db.export_attributes()

    def buffers():
        return dict(rows=np.zeros(n_mp, TRACK_DTYPE), status=np.zeros(n_mp, np.uint8), taken=s["taken"].copy(), assigned=np.full(n_kp, -1, np.int32),
                    n_to=C.c_int32(0), n_m=C.c_int32(0))

    a, b, c = buffers(), buffers(), buffers()
    part = dict(gather=[], flat=[], resident=[], stage=[], restaged=[])
    g = {}

    def flat():
        a["taken"][:], a["assigned"][:] = s["taken"], -1
        t0 = time.perf_counter()
        g["pos_min"] = np.concatenate([pos[slots], (np.float32(0.8) * mn[slots])[:, None]], axis=1)
        g["normal_max"] = np.concatenate([normal[slots], (np.float32(1.2) * mx[slots])[:, None]], axis=1)
        g["max"], g["desc"], g["has"] = mx[slots], desc[slots], has_map[slots]
        table = y._lib.YdMapPointTable(p(g["pos_min"]), p(g["normal_max"]), p(g["max"]), p(g["desc"]), n_mp)
        t1 = time.perf_counter()
        assert L.ydorb_search_local_points(m._h, C.byref(fv), C.byref(view), C.byref(table), p(s["skip"]), p(g["has"]), TH, RATIO, p(a["taken"]),
                                           p(a["assigned"]), p(a["rows"]), p(a["status"]), C.byref(a["n_to"]), C.byref(a["n_m"])) == 0
        part["gather"].append(t1 - t0); part["flat"].append(time.perf_counter() - t0)

    def call(d):
        assert L.ydorb_mapdb_search_local_points(db._h, m._h, C.byref(fv), C.byref(view), p(slots), n_mp, p(s["skip"]), TH, RATIO, p(d["taken"]),
                                                 p(d["assigned"]), p(d["rows"]), p(d["status"]), C.byref(d["n_to"]), C.byref(d["n_m"])) == 0

    def resident():
        b["taken"][:], b["assigned"][:] = s["taken"], -1
        t0 = time.perf_counter()
        call(b)
        part["resident"].append(time.perf_counter() - t0)

    nrm, mns, mxs, dsc = normal[slots], mn[slots], mx[slots], desc[slots]

    def restaged():
        c["taken"][:], c["assigned"][:] = s["taken"], -1
        t0 = time.perf_counter()
        assert L.ydorb_mapdb_set_point_attributes(db._h, p(slots), n_mp, p(nrm), p(mns), p(mxs), p(dsc)) == 0
        t1 = time.perf_counter()
        call(c)
        part["stage"].append(t1 - t0); part["restaged"].append(time.perf_counter() - t0)

    def check():
        flat(); resident(); restaged()
        for d in (b, c):
            assert a["rows"].tobytes() == d["rows"].tobytes() and np.array_equal(a["status"], d["status"]) and np.array_equal(a["assigned"], d["assigned"])
            assert np.array_equal(a["taken"], d["taken"]) and a["n_m"].value == d["n_m"].value and a["n_to"].value == d["n_to"].value

    check()
    for _ in range(5):
        flat(); resident(); restaged()
    for v in part.values():
        v.clear()
    for _ in range(REPS):                                   # the variants alternate within each repetition
        flat(); resident(); restaged()
    out = {k + "_ms": [round(float(x) * 1e3, 4) for x in (np.median(v), min(v), max(v))] for k, v in part.items()}
    restaged_bytes = db.attr_stats()["last_attr_sync_bytes"]
    resident()
    assert db.attr_stats()["last_attr_sync_bytes"] == 0 and db.stats()["last_sync_bytes"] == 0
    for d in (a, b, c):
        d["rows"][:], d["status"][:] = 0, 9
    check()
    frame_bytes = n_kp * (s["kps"].itemsize + 32 + 4 + 1 + 4)   # keypoints, descriptors, right x, taken, assigned: the same on every path
    out["upload_bytes"] = dict(frame=frame_bytes, flat_map=n_mp * (16 + 16 + 4 + 32 + 1 + 1), resident_map=n_mp * (4 + 1),
                               restaged_map=n_mp * (4 + 1) + restaged_bytes)
    out["in_view"], out["matches"] = a["n_to"].value, a["n_m"].value
    db.close()
    return out


def main():
    L, R = y.lib(), S.ref()
    if "--resident" in sys.argv[1:]:
        m = y.OrbMatcher(RATIO, check_orientation=False)
        out = {"metric": "resident_search_local_points_ms", "th": TH, "reps": REPS, "search": {}}
        for n_kp in (1000, 2000):
            for n_mp in (300, 2000, 8000):
                out["search"]["kp%d_mp%d" % (n_kp, n_mp)] = resident_case(L, m, n_kp, n_mp)
        m.close()
        print(json.dumps(out))
        return
    m = y.OrbMatcher(RATIO, check_orientation=False)
    out = {"metric": "search_local_points_ms", "th": TH, "reps": REPS, "search": {}, "cull": {}}
    for n_kp in (1000, 2000):
        for n_mp in (1000, 3000, 8000):
            out["search"]["kp%d_mp%d" % (n_kp, n_mp)] = search_case(L, R, m, n_kp, n_mp)
    for n_views in (1, 8, 64):
        out["cull"]["views%d" % n_views] = cull_case(L, R, n_views)
    m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
