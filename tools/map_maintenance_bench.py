"""Time of the three map-maintenance entries (ydorb_map_update_normal_depth, ydorb_map_covisibility, ydorb_map_keyframe_redundancy), host
to host at the C entry points on arrays prepared once, against the CPU restatement (tests/mapmaint_ref, one thread) on the same
flattened arrays in the same run, at two sizes:
  local  LocalMapping's: 31 keyframes of about 1500 map points each, 4-8 observers per point (about 7 750 points);
  map    a whole map: 5000 keyframes, 400 000 points, 4-8 observers from a window of 31 neighbouring keyframes.
Median wall time of the synchronous calls after warm-up with [min, max] beside it; the outputs of both sides are compared exactly
before timing.  Flat arrays flatter the CPU side against the reference's mutex-guarded containers, and the adapters' flattening is
outside both figures: --flatten runs tests/cpp_host/mapmaint_run.cpp on the local size and reports its host time per flattening.
The kernels alone: run this tool under `rocprofv3 --kernel-trace --stats -- python tools/map_maintenance_bench.py --size local` (and
`--size map`) and read the k_normal_depth / k_covisibility / k_redundancy rows; --kernel-ms NAME=MS turns such a figure into the
normal-and-depth kernel's achieved bytes per second.
--resident times the resident map table (ydorb_mapdb_*) instead: the map-size table is loaded into one handle
once; then, per repetition and alternating with the flat entry on the same data, the resident normal-and-depth call for the local
window's 7 750 points after 0, 300 and 7 750 of them were touched (staging and query timed apart), and the resident covisibility and
redundancy calls for the local window's lists; outputs are compared exactly before timing.  Two further handles, created without
spare pool room, each time one query that has to repack: the map-size table, and 20 000 points of 300 observers.  It ends with tests/cpp_host/mapdb_run.cpp
on local-size stand-ins: the three adapters through MapMirror beside the flattening adapters, and the price of a flush.  The kernels
k_mapdb_apply / k_mapdb_repack: `rocprofv3 --kernel-trace --stats -- python tools/map_maintenance_bench.py --resident --reps 5`.
--correct times the map correction on the resident table (ydorb_mapdb_correct) beside the route it replaces, for
the three loops of loop closing; see bench_correct.  Its kernels k_mapdb_correct / k_mapdb_correct_centres: the same rocprofv3 line
with --correct.
--local-map times the two set queries of Tracking::updateLocalMap on the resident table's keyframe rows; see
bench_local_map.  Its kernels k_rowset_mark / _count / _emit and the int instantiation of k_mapdb_span_apply / _repack (the trace
names them k_mapdb_span_apply<int, 1> / k_mapdb_span_repack<int, 1>): the same rocprofv3 line with --local-map.
--descriptors times MapPoint::computeDistinctiveDescriptors on the resident table's descriptor blocks and point views (DESIGN.md section
6p) beside the flat path as a caller must run it and the CPU oracle; see bench_descriptors.  Its kernels k_mapdb_distinctive and
k_mapdb_span_apply / _repack (<uint4, 2> for the blocks, <int, 1> for the views): the same rocprofv3 line with --descriptors.
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mapmaint_support as S  # noqa: E402
import ydorbslam_amd as y  # noqa: E402
from ydorbslam_amd import map_maintenance as M  # noqa: E402

p = lambda a: a.ctypes.data_as(C.c_void_p)
SIZES = dict(local=(31, 7750, 31), map=(5000, 400000, 31))


def times(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return [round(float(v) * 1e3, 4) for v in (np.median(ts), min(ts), max(ts))]


def make_map(n_kf, n_points, window, seed=1):
    """Flat arrays of a map whose points are seen by 4-8 distinct keyframes out of `window` consecutive ones, in a shuffled order."""
    rng = np.random.default_rng(seed)
    m = rng.integers(4, 9, n_points)
    base = rng.integers(0, max(n_kf - window, 0) + 1, n_points)
    pick = np.argsort(rng.uniform(size=(n_points, window)), axis=1)[:, :8]          # 8 distinct offsets per point, shuffled
    keep = np.arange(8)[None, :] < m[:, None]
    obs_kf = (base[:, None] + pick)[keep].astype(np.int32)
    obs_start = np.concatenate([[0], np.cumsum(m)]).astype(np.int32)
    point_of = np.repeat(np.arange(n_points, dtype=np.int32), m)
    lvl_base = rng.integers(0, 8, n_points)
    level = np.clip(lvl_base[point_of] + rng.integers(-1, 2, len(obs_kf)), 0, 7).astype(np.uint8)
    stereo = rng.uniform(size=len(obs_kf)) < 0.5
    T = M.ObservationTable.from_arrays(n_kf, obs_start, obs_kf, level | np.where(stereo, 0x80, 0).astype(np.uint8),
                                       (rng.uniform(size=n_points) < 0.02).astype(np.uint8))
    by_kf = np.argsort(obs_kf, kind="stable")                                      # each keyframe's map-point vector
    kf_start = np.concatenate([[0], np.cumsum(np.bincount(obs_kf, minlength=n_kf))]).astype(np.int32)
    first = obs_start[:-1]
    return dict(T=T, pos=(rng.uniform(-6, 6, (n_points, 3)) + [0, 0, 12]).astype(np.float32), centre=rng.uniform(-4, 4, (n_kf, 3)).astype(np.float32),
                ref_kf=np.ascontiguousarray(obs_kf[first]), ref_level=np.ascontiguousarray(level[first]), kf_start=kf_start,
                kf_points=np.ascontiguousarray(point_of[by_kf]), kf_levels=np.ascontiguousarray(level[by_kf]), n_obs=len(obs_kf))


def bench_size(name, reps):
    n_kf, n_points, window = SIZES[name]
    L, R = y.lib(), S.ref()
    d = make_map(n_kf, n_points, window)
    T, sf = d["T"], S.scale_factors()
    out = dict(keyframes=n_kf, points=n_points, observations=d["n_obs"])

    def both(label, gpu_fn, ref_fn, make_args, outputs):
        a, b = make_args(), make_args()
        assert gpu_fn(*a) == 0, L.ydorb_last_error()
        assert ref_fn(*b) == 0
        for k in outputs:
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (label, k)
        out[label] = dict(gpu_ms=times(lambda: gpu_fn(*a), reps), cpu_ms=times(lambda: ref_fn(*b), max(3, reps // 3)))

    class Args(list):   # ctypes arguments that keep their numpy arrays reachable by position
        def __init__(self, items):
            super().__init__(items)
            self.c = [p(v) if isinstance(v, np.ndarray) else v for v in items]

        def __iter__(self):
            return iter(self.c)

    def nd_args():
        return Args([C.byref(T.struct), d["pos"], d["centre"], d["ref_kf"], d["ref_level"], sf, 8, 0, np.zeros((n_points, 3), np.float32),
                     np.zeros(n_points, np.float32), np.zeros(n_points, np.float32), np.zeros(n_points, np.uint8)])

    both("normal_depth", L.ydorb_map_update_normal_depth, R.mapref_update_normal_depth, nd_args, (8, 9, 10, 11))
    out["normal_depth"]["algorithmic_bytes"] = int(n_points * (8 + 12 + 4 + 1 + 1 + 21) + d["n_obs"] * (4 + 12))

    def lists(kfs):
        start = np.concatenate([[0], np.cumsum(d["kf_start"][kfs + 1] - d["kf_start"][kfs])]).astype(np.int32)
        idx = np.concatenate([d["kf_points"][d["kf_start"][k]:d["kf_start"][k + 1]] for k in kfs]).astype(np.int32)
        own = np.concatenate([d["kf_levels"][d["kf_start"][k]:d["kf_start"][k + 1]] for k in kfs]).astype(np.uint8)
        return start, np.ascontiguousarray(idx), np.ascontiguousarray(own)

    for label, q in (("covisibility_1", np.array([n_kf // 2], np.int32)), ("covisibility_all", np.arange(n_kf, dtype=np.int32))):
        start, idx, _ = lists(q)
        span = T.span_lengths()
        caps = [min(n_kf - 1, int(span[idx[start[i]:start[i + 1]]].sum())) for i in range(len(q))]
        out_start = np.concatenate([[0], np.cumsum(caps)]).astype(np.int32)

        def cv_args():
            return Args([C.byref(T.struct), q, len(q), start, idx, out_start, 0, np.full(max(int(out_start[-1]), 1), -1, np.int32),
                         np.full(max(int(out_start[-1]), 1), -1, np.int32), np.zeros(len(q), np.int32), np.zeros(len(q), np.uint8)])

        both(label, L.ydorb_map_covisibility, R.mapref_covisibility, cv_args, (7, 8, 9, 10))
        out[label]["queries"], out[label]["list_entries"] = len(q), int(start[-1])

    cand = np.arange(1, n_kf, dtype=np.int32)
    start, idx, own = lists(cand)
    removed = np.zeros(n_kf, np.uint8)
    removed[cand[::7]] = 1
    for label, rem in (("redundancy", None), ("redundancy_masked", removed)):
        def rd_args():
            return Args([C.byref(T.struct), cand, len(cand), start, idx, own, rem, 3, 0, np.zeros(len(cand), np.int32), np.zeros(len(cand), np.int32),
                         np.zeros(len(cand), np.uint8)])

        both(label, L.ydorb_map_keyframe_redundancy, R.mapref_keyframe_redundancy, rd_args, (9, 10, 11))
        out[label]["candidates"], out[label]["list_entries"] = len(cand), int(start[-1])
    return out


def stat(ts):
    return [round(float(v) * 1e3, 4) for v in (np.median(ts), min(ts), max(ts))]


def bench_resident(reps):
    import mapdb_support as D
    from ydorbslam_amd._lib import YdMapDbStats
    n_kf, n_points, window = SIZES["map"]
    L = y.lib()
    d = make_map(n_kf, n_points, window)
    T, sf = d["T"], S.scale_factors()
    out = dict(keyframes=n_kf, points=n_points, observations=d["n_obs"])
    h = C.c_void_p()
    y._lib.check(L.ydorb_mapdb_create(0, n_points, n_kf, 2 * d["n_obs"], C.byref(h)))
    all_slots, kf_slots = np.arange(n_points, dtype=np.int32), np.arange(n_kf, dtype=np.int32)

    def stats():
        st = YdMapDbStats()
        L.ydorb_mapdb_stats(h, C.byref(st))
        return {k: int(getattr(st, k)) for k, _ in YdMapDbStats._fields_}

    def set_points(slots):
        """Re-sends the records of `slots` (ascending) as they are."""
        m = np.diff(T.obs_start.astype(np.int64))[slots]
        start = np.concatenate([[0], np.cumsum(m)]).astype(np.int32)
        take = np.concatenate([np.arange(T.obs_start[p], T.obs_start[p + 1]) for p in slots]) if len(slots) else np.zeros(0, np.int64)
        args = [np.ascontiguousarray(a) for a in (slots, start, T.obs_kf[take], T.obs_level[take], T.bad[slots], d["ref_kf"][slots], d["ref_level"][slots], d["pos"][slots])]
        return lambda: L.ydorb_mapdb_set_points(h, p(args[0]), len(slots), *[p(a) for a in args[1:]]), args

    t0 = time.perf_counter()
    assert L.ydorb_mapdb_set_centres(h, p(kf_slots), n_kf, p(d["centre"])) == 0
    assert L.ydorb_mapdb_set_points(h, p(all_slots), n_points, p(T.obs_start), p(T.obs_kf), p(T.obs_level), p(T.bad), p(d["ref_kf"]), p(d["ref_level"]), p(d["pos"])) == 0, L.ydorb_last_error()
    k0 = n_kf // 2
    local_kfs = np.arange(k0, k0 + window, dtype=np.int32)
    # the local window's 7 750 points: keyframes of the map-size table hold fewer points each, so the window's points are those of as
    # many neighbouring keyframes as it takes
    wide = np.arange(k0, min(k0 + 4 * window, n_kf))
    local = np.unique(np.concatenate([d["kf_points"][d["kf_start"][k]:d["kf_start"][k + 1]] for k in wide]))[:SIZES["local"][1]].astype(np.int32)
    n = len(local)
    res = [np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint8)]
    resident_nd = lambda: L.ydorb_mapdb_update_normal_depth(h, p(local), n, p(sf), 8, *[p(a) for a in res])
    assert resident_nd() == 0, L.ydorb_last_error()
    out["load_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    out["load_sync_bytes"] = stats()["last_sync_bytes"]
    flat = [np.zeros((n_points, 3), np.float32), np.zeros(n_points, np.float32), np.zeros(n_points, np.float32), np.zeros(n_points, np.uint8)]
    flat_nd = lambda: L.ydorb_map_update_normal_depth(C.byref(T.struct), p(d["pos"]), p(d["centre"]), p(d["ref_kf"]), p(d["ref_level"]), p(sf), 8, 0, *[p(a) for a in flat])
    assert flat_nd() == 0
    for a, b in zip(res, flat):
        assert np.array_equal(a.view(np.uint8), b[local].view(np.uint8))
    # the flat entry over the local window alone: a table of the local points over the same keyframe slots
    m = np.diff(T.obs_start.astype(np.int64))[local]
    take = np.concatenate([np.arange(T.obs_start[q], T.obs_start[q + 1]) for q in local])
    TL = M.ObservationTable.from_arrays(n_kf, np.concatenate([[0], np.cumsum(m)]).astype(np.int32), T.obs_kf[take], T.obs_level[take], T.bad[local])
    lpos, lref, llvl = [np.ascontiguousarray(d[k][local]) for k in ("pos", "ref_kf", "ref_level")]
    fl = [np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint8)]
    flat_local = lambda: L.ydorb_map_update_normal_depth(C.byref(TL.struct), p(lpos), p(d["centre"]), p(lref), p(llvl), p(sf), 8, 0, *[p(a) for a in fl])
    assert flat_local() == 0
    for a, b in zip(res, fl):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    rows = {}
    for touched in (0, 300, n):
        stage, keep = set_points(local[:touched])
        ts = dict(stage=[], query=[], flat_map=[], flat_local=[])
        sync_bytes = 0
        for r in range(reps + 1):
            t = [time.perf_counter()]
            if touched:
                assert stage() == 0
            t.append(time.perf_counter())
            assert resident_nd() == 0
            t.append(time.perf_counter())
            sync_bytes = stats()["last_sync_bytes"]
            u = [time.perf_counter()]
            flat_nd()
            u.append(time.perf_counter())
            flat_local()
            u.append(time.perf_counter())
            if r:
                ts["stage"].append(t[1] - t[0]); ts["query"].append(t[2] - t[1]); ts["flat_map"].append(u[1] - u[0]); ts["flat_local"].append(u[2] - u[1])
        for a, b in zip(res, fl):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        rows["touched_%d" % touched] = dict(stage_ms=stat(ts["stage"]), resident_query_ms=stat(ts["query"]), flat_map_ms=stat(ts["flat_map"]),
                                            flat_local_ms=stat(ts["flat_local"]), sync_bytes=sync_bytes)
    out["normal_depth_local_points"] = dict(points=n, **rows)

    # covisibility and redundancy of the local window's lists against the map-size table
    start = np.concatenate([[0], np.cumsum(d["kf_start"][local_kfs + 1] - d["kf_start"][local_kfs])]).astype(np.int32)
    idx = np.ascontiguousarray(np.concatenate([d["kf_points"][d["kf_start"][k]:d["kf_start"][k + 1]] for k in local_kfs]).astype(np.int32))
    own = np.ascontiguousarray(np.concatenate([d["kf_levels"][d["kf_start"][k]:d["kf_start"][k + 1]] for k in local_kfs]).astype(np.uint8))
    span = T.span_lengths()
    caps = [min(n_kf - 1, int(span[idx[start[i]:start[i + 1]]].sum())) for i in range(window)]
    out_start = np.concatenate([[0], np.cumsum(caps)]).astype(np.int32)
    tot = int(out_start[-1])
    mk = lambda: [np.full(tot, -1, np.int32), np.full(tot, -1, np.int32), np.zeros(window, np.int32), np.zeros(window, np.uint8)]
    ra, fa = mk(), mk()
    pairs = dict(covisibility=(lambda: L.ydorb_mapdb_covisibility(h, p(local_kfs), window, p(start), p(idx), p(out_start), *[p(a) for a in ra]),
                               lambda: L.ydorb_map_covisibility(C.byref(T.struct), p(local_kfs), window, p(start), p(idx), p(out_start), 0, *[p(a) for a in fa]), ra, fa))
    rb, fb = [np.zeros(window, np.int32), np.zeros(window, np.int32), np.zeros(window, np.uint8)], [np.zeros(window, np.int32), np.zeros(window, np.int32), np.zeros(window, np.uint8)]
    pairs["redundancy"] = (lambda: L.ydorb_mapdb_keyframe_redundancy(h, p(local_kfs), window, p(start), p(idx), p(own), None, 3, *[p(a) for a in rb]),
                           lambda: L.ydorb_map_keyframe_redundancy(C.byref(T.struct), p(local_kfs), window, p(start), p(idx), p(own), None, 3, 0, *[p(a) for a in fb]), rb, fb)
    for label, (rf, ff, ro, fo) in pairs.items():
        assert rf() == 0 and ff() == 0, L.ydorb_last_error()
        for a, b in zip(ro, fo):
            assert np.array_equal(a, b), label
        tr, tf = [], []
        for r in range(reps + 1):
            t0 = time.perf_counter(); rf(); t1 = time.perf_counter(); ff(); t2 = time.perf_counter()
            if r:
                tr.append(t1 - t0); tf.append(t2 - t1)
        out[label + "_local_lists"] = dict(queries=window, list_entries=int(start[-1]), resident_ms=stat(tr), flat_map_ms=stat(tf))
    # one repack at the map size, once: a second handle whose pool has no room for the 7 750 re-sent spans
    h2 = C.c_void_p()
    y._lib.check(L.ydorb_mapdb_create(0, n_points, n_kf, d["n_obs"] + 1000, C.byref(h2)))
    L.ydorb_mapdb_set_centres(h2, p(kf_slots), n_kf, p(d["centre"]))
    L.ydorb_mapdb_set_points(h2, p(all_slots), n_points, p(T.obs_start), p(T.obs_kf), p(T.obs_level), p(T.bad), p(d["ref_kf"]), p(d["ref_level"]), p(d["pos"]))
    again = lambda: L.ydorb_mapdb_update_normal_depth(h2, p(local), n, p(sf), 8, *[p(a) for a in res])
    assert again() == 0
    _, args = set_points(local)
    assert L.ydorb_mapdb_set_points(h2, p(args[0]), n, *[p(a) for a in args[1:]]) == 0
    t0 = time.perf_counter()
    assert again() == 0
    t1 = time.perf_counter()
    st2 = YdMapDbStats()
    L.ydorb_mapdb_stats(h2, C.byref(st2))
    out["query_with_a_repack_at_map_size"] = dict(ms_once=round((t1 - t0) * 1e3, 4), repacks_grown=int(st2.repacks_grown), sync_bytes=int(st2.last_sync_bytes),
                                                  pool_capacity=int(st2.pool_capacity))
    for a, b in zip(res, fl):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    L.ydorb_mapdb_destroy(h2)
    # ... and one repack of long spans: 20 000 points of 300 observers each, the pool again without room
    rng = np.random.default_rng(3)
    nl, ll = 20000, 300
    lkf = np.ascontiguousarray(np.argsort(rng.uniform(size=(nl, 512)), axis=1)[:, :ll].astype(np.int32).reshape(-1) + rng.integers(0, n_kf - 512, nl).repeat(ll).astype(np.int32))
    lstart = (np.arange(nl + 1, dtype=np.int64) * ll).astype(np.int32)
    llev, lbad, lslots = np.zeros(nl * ll, np.uint8), np.zeros(nl, np.uint8), np.arange(nl, dtype=np.int32)
    lref, lrl, lp = np.ascontiguousarray(lkf[::ll]), np.zeros(nl, np.uint8), np.ascontiguousarray(d["pos"][:nl])
    h3 = C.c_void_p()
    y._lib.check(L.ydorb_mapdb_create(0, nl, n_kf, nl * ll + 1000, C.byref(h3)))
    L.ydorb_mapdb_set_centres(h3, p(kf_slots), n_kf, p(d["centre"]))
    assert L.ydorb_mapdb_set_points(h3, p(lslots), nl, p(lstart), p(lkf), p(llev), p(lbad), p(lref), p(lrl), p(lp)) == 0, L.ydorb_last_error()
    some = np.arange(100, dtype=np.int32)
    lres = [np.zeros((100, 3), np.float32), np.zeros(100, np.float32), np.zeros(100, np.float32), np.zeros(100, np.uint8)]
    ask = lambda: L.ydorb_mapdb_update_normal_depth(h3, p(some), 100, p(sf), 8, *[p(a) for a in lres])
    assert ask() == 0
    before = [a.copy() for a in lres]
    assert L.ydorb_mapdb_set_points(h3, p(some), 100, p(lstart[:101]), p(lkf[:100 * ll]), p(llev), p(lbad), p(lref), p(lrl), p(lp)) == 0
    t0 = time.perf_counter()
    assert ask() == 0
    t1 = time.perf_counter()
    L.ydorb_mapdb_stats(h3, C.byref(st2))
    for a, b in zip(lres, before):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    out["query_with_a_repack_of_long_spans"] = dict(points=nl, span=ll, ms_once=round((t1 - t0) * 1e3, 4), repacks_grown=int(st2.repacks_grown))
    L.ydorb_mapdb_destroy(h3)
    st = stats()
    out["handle"] = {k: st[k] for k in ("pool_used", "pool_capacity", "repacks_kept", "repacks_grown", "point_table_growths", "keyframe_table_growths")}
    L.ydorb_mapdb_destroy(h)

    # adapter level, on stand-ins at the local size
    m = S.random_map(5, 31, 7750, 4, 8, level_spread=1)
    scene = S.adapter_scene(m, 8.0, seed=2)
    tmp = tempfile.mkdtemp(prefix="mdbench")
    exe = D.build_mirror_exe(os.path.join(tmp, "mapdb_run"))
    run = D.run_mirror(exe, tmp, scene, 0, list(range(31)), [15], S.scale_factors(), reps=reps)
    assert all(run[ph + k] == 1 for ph in "ABC" for k in ("_normal_same", "_covisibility_same", "_culling_same"))
    out["adapters_local_stand_ins_ms"] = {k[len("time_"):-len("_ms")]: v for k, v in run.items() if k.startswith("time_")}
    return out


def bench_correct(reps):
    """ydorb_mapdb_correct against the route it replaces, alternating in one run on two handles that hold the same
    map-size table: the restatement's host loop for the positions (tests/mapcorrect_ref, one thread, flat arrays), then
    ydorb_mapdb_set_positions, ydorb_mapdb_set_centres and ydorb_mapdb_update_normal_depth.  Shape A: loop A on the 31-keyframe window;
    B: loop B on the whole map; C: loop C on the whole map (no normals; the old route's staged positions are landed by a one-point
    query).  The transforms are small, so that the repetitions do not carry the map away.  With complete map-point lists no point of loop A
    has an observer before its corrector, so the old route reproduces A's normals by asking for them before it sets the centres."""
    import mapcorrect_support as K
    from ydorbslam_amd.map_resident import correction
    n_kf, n_points, window = SIZES["map"]
    L, R = y.lib(), K.ref()
    d = make_map(n_kf, n_points, window)
    T, sf = d["T"], S.scale_factors()
    out = dict(keyframes=n_kf, points=n_points, observations=d["n_obs"])
    all_slots, kf_all = np.arange(n_points, dtype=np.int32), np.arange(n_kf, dtype=np.int32)
    hs = []
    for _ in range(2):
        h = C.c_void_p()
        y._lib.check(L.ydorb_mapdb_create(0, n_points, n_kf, d["n_obs"] + 1000, C.byref(h)))
        assert L.ydorb_mapdb_set_centres(h, p(kf_all), n_kf, p(d["centre"])) == 0
        assert L.ydorb_mapdb_set_points(h, p(all_slots), n_points, p(T.obs_start), p(T.obs_kf), p(T.obs_level), p(T.bad), p(d["ref_kf"]), p(d["ref_level"]), p(d["pos"])) == 0
        hs.append(h)
    new, old = hs
    rng = np.random.default_rng(7)

    def small_sim3(k):
        before, _ = K.sim3_pairs(11, k)
        after = before.copy()
        after[:, :4] += rng.uniform(-1e-3, 1e-3, (k, 4))
        after[:, :4] /= np.linalg.norm(after[:, :4], axis=1, keepdims=True)
        after[:, 4:7] += rng.uniform(-1e-2, 1e-2, (k, 3))
        after[:, 7] = rng.uniform(0.999, 1.001, k)
        return before, after

    k0 = n_kf // 2
    win = np.arange(k0, k0 + window, dtype=np.int32)
    a_slots = np.concatenate([d["kf_points"][d["kf_start"][k]:d["kf_start"][k + 1]] for k in win]).astype(np.int32)
    a_corr = np.concatenate([np.full(d["kf_start"][k + 1] - d["kf_start"][k], r, np.int32) for r, k in enumerate(win)])
    ba, aa = small_sim3(window)
    bb, ab = small_sim3(n_kf)
    reached = np.setdiff1d(kf_all, kf_all[::50]).astype(np.int32)
    bc, ac = K.se3_pairs(5, len(reached))
    for i in range(len(reached)):                                  # after = the inverse of before, moved a little: the map stays in place
        Rcw, tcw = bc[i, :9].reshape(3, 3).astype(np.float64), bc[i, 9:].astype(np.float64)
        ac[i, :9], ac[i, 9:] = Rcw.T.reshape(-1), -Rcw.T @ tcw + rng.uniform(-1e-2, 1e-2, 3)
    cen = lambda kfs, s: (d["centre"][kfs] + np.random.default_rng(s).uniform(-0.05, 0.05, (len(kfs), 3))).astype(np.float32)
    shapes = dict(
        A=dict(kf_slots=win, before=ba, after=aa, slots=a_slots, corrector=a_corr, arithmetic="sim3", centre_after=cen(win, 1), centres="interleaved", scale_factors=sf),
        B=dict(kf_slots=kf_all, before=bb, after=ab, slots=None, corrector=None, arithmetic="sim3", centre_after=cen(kf_all, 2), centres="poses_first", scale_factors=sf),
        C=dict(kf_slots=reached, before=bc, after=ac, slots=None, corrector=None, arithmetic="se3", centre_after=None, centres="resident", scale_factors=None))
    flat = dict(table=T, pos=d["pos"].copy(), centre=d["centre"].copy(), ref_kf=d["ref_kf"], ref_level=d["ref_level"])
    one = np.zeros(1, np.int32)
    one_out = [np.zeros((1, 3), np.float32), np.zeros(1, np.float32), np.zeros(1, np.float32), np.zeros(1, np.uint8)]
    for name, args in shapes.items():
        corr, res, _keep = correction(args["kf_slots"], args["before"], args["after"], n_points if args["slots"] is None else None, args["slots"],
                                      args["corrector"], args["arithmetic"], args["centre_after"], args["centres"], args["scale_factors"])
        # the old route's host loop: the same call without normals, on the flat arrays
        hcorr, hres, _hkeep = correction(args["kf_slots"], args["before"], args["after"], n_points if args["slots"] is None else None, args["slots"],
                                         args["corrector"], args["arithmetic"], args["centre_after"], "resident", None)
        n = len(res["status"])
        slots = all_slots if args["slots"] is None else args["slots"]
        nd = [np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint8)]
        K_ = len(args["kf_slots"])

        def new_route():
            assert L.ydorb_mapdb_correct(new, C.byref(corr)) == 0, L.ydorb_last_error()

        def old_route():
            assert R.mapcorrect_ref(C.byref(T.struct), p(flat["pos"]), p(flat["centre"]), p(flat["ref_kf"]), p(flat["ref_level"]), C.byref(hcorr)) == 0
            done = np.flatnonzero((hres["status"] == 0) | (hres["status"] == 4))
            moved = np.ascontiguousarray(slots[done])
            moved_pos = np.ascontiguousarray(hres["pos"][done])
            if name == "B":
                assert L.ydorb_mapdb_set_centres(old, p(args["kf_slots"]), K_, p(args["centre_after"])) == 0
            assert L.ydorb_mapdb_set_positions(old, p(moved), len(moved), p(moved_pos)) == 0
            if name == "C":
                assert L.ydorb_mapdb_update_normal_depth(old, p(one), 1, p(sf), 8, *[p(a) for a in one_out]) == 0
                return done
            assert L.ydorb_mapdb_update_normal_depth(old, p(slots), n, p(sf), 8, *[p(a) for a in nd]) == 0, L.ydorb_last_error()
            if name == "A":
                assert L.ydorb_mapdb_set_centres(old, p(args["kf_slots"]), K_, p(args["centre_after"])) == 0
            return done

        tn, to = [], []
        for r in range(reps + 1):
            t0 = time.perf_counter(); new_route(); t1 = time.perf_counter(); done = old_route(); t2 = time.perf_counter()
            if r == 0:                                             # the two routes agree exactly before anything is timed
                assert np.array_equal(res["pos"].view(np.uint32), hres["pos"].view(np.uint32)), name
                if name != "C":
                    for k, a in zip(("normal", "min_distance", "max_distance"), nd):
                        assert np.array_equal(res[k][done].view(np.uint32), a[done].view(np.uint32)), (name, k)
            else:
                tn.append(t1 - t0); to.append(t2 - t1)
        nc = int(len(done))
        per_kf = 64 if args["arithmetic"] == "sim3" else 48
        up = 2 * per_kf * K_ + 4 * n_kf + 4 * K_ + (12 * K_ if args["centre_after"] is not None else 0) + 8 * nc
        down = nc * (13 + (20 if args["scale_factors"] is not None else 0))
        old_up = 16 * nc + (16 * K_ if args["centre_after"] is not None else 0) + (4 * n if name != "C" else 4)
        old_down = 21 * n if name != "C" else 21
        out[name] = dict(entries=int(n), corrected=nc, keyframes=K_, correct_ms=stat(tn), previous_route_ms=stat(to), correct_bytes_up=up, correct_bytes_down=down,
                         previous_route_bytes_up=old_up, previous_route_bytes_down=old_down)
    ex = []
    for h in hs:                                                   # and the two tables ended up the same
        pos, centre = np.zeros((n_points, 3), np.float32), np.zeros((n_kf, 3), np.float32)
        st, kf, lv = np.zeros(n_points + 1, np.int32), np.zeros(d["n_obs"], np.int32), np.zeros(d["n_obs"], np.uint8)
        bad, rk, rl = np.zeros(n_points, np.uint8), np.zeros(n_points, np.int32), np.zeros(n_points, np.uint8)
        assert L.ydorb_mapdb_export(h, p(st), p(kf), p(lv), p(bad), p(rk), p(rl), p(pos), p(centre)) == 0
        ex.append((pos, centre))
        L.ydorb_mapdb_destroy(h)
    out["tables_equal_afterwards"] = bool(np.array_equal(ex[0][0].view(np.uint32), ex[1][0].view(np.uint32)) and
                                          np.array_equal(ex[0][1].view(np.uint32), ex[1][1].view(np.uint32)))
    assert out["tables_equal_afterwards"]
    return out


def bench_local_map(reps):
    """--local-map: the two set queries of Tracking::updateLocalMap on the resident table's keyframe rows beside
    the host restatement of the two reference loops (tests/localmap_ref, one thread, flat arrays) on the same data, alternating in one
    process.  The map-size table and every keyframe's row (the map's own density) are loaded once; the window is 80 keyframes round
    keyframe 2 500.  Timed: points_of_keyframes with nothing staged and with 200 row entries staged (staging + query), the observer
    counter of one frame of 1 000 points, and the same points query over synthetic rows of 2 000 entries, half of them null.  Outputs are
    compared exactly before and after timing.  It ends with tests/cpp_host/localmap_run.cpp: updateLocalKeyFramesImpl / updateLocalPointsImpl
    through MapMirror beside the two reference loops on the same stand-ins, alternating."""
    import mapdb_rows_support as R
    n_kf, n_points, window = SIZES["map"]
    L, ref = y.lib(), R.ref()
    d = make_map(n_kf, n_points, window)
    T = d["T"]
    db = y.MapDb(0, n_points, n_kf, 2 * d["n_obs"])
    h = db._h
    all_slots, kf_slots = np.arange(n_points, dtype=np.int32), np.arange(n_kf, dtype=np.int32)
    assert L.ydorb_mapdb_set_centres(h, p(kf_slots), n_kf, p(d["centre"])) == 0
    assert L.ydorb_mapdb_set_points(h, p(all_slots), n_points, p(T.obs_start), p(T.obs_kf), p(T.obs_level), p(T.bad), p(d["ref_kf"]), p(d["ref_level"]), p(d["pos"])) == 0
    out = dict(keyframes=n_kf, points=n_points, observations=d["n_obs"], reps=reps)
    rng = np.random.default_rng(7)
    win = np.arange(n_kf // 2 - 40, n_kf // 2 + 40, dtype=np.int32)

    def run(tag, row_start, row_slot):
        """One row configuration: row_start [n_kf + 1] / row_slot for every keyframe slot."""
        row_start, row_slot = np.ascontiguousarray(row_start, np.int32), np.ascontiguousarray(row_slot, np.int32)
        t0 = time.perf_counter()
        assert L.ydorb_mapdb_set_keyframe_rows(h, p(kf_slots), n_kf, p(row_start), p(row_slot)) == 0, L.ydorb_last_error()
        got_rows = db.export_rows()
        load_ms = (time.perf_counter() - t0) * 1e3
        assert all(np.array_equal(got_rows[k], row_slot[row_start[k]:row_start[k + 1]]) for k in win)
        E = int(sum(row_start[k + 1] - row_start[k] for k in win))
        own = np.concatenate([row_slot[row_start[k]:row_start[k + 1]] for k in win[38:43]])
        frame = np.ascontiguousarray(np.concatenate([own[own >= 0][:900], np.full(100, -1, np.int32)]), np.int32)   # one frame: 1 000 entries, 100 without a point
        cap = min(E, n_points)
        g_out, g_seen, r_out, r_seen = np.zeros(cap, np.int32), np.zeros(cap, np.uint8), np.zeros(cap, np.int32), np.zeros(cap, np.uint8)
        cnt, st = C.c_int32(0), C.c_uint8(0)

        def gpu_points():
            assert L.ydorb_mapdb_points_of_keyframes(h, p(win), len(win), p(frame), len(frame), cap, p(g_out), p(g_seen), C.byref(cnt), C.byref(st)) == 0

        def ref_points():
            return ref.localmapref_points_of_keyframes(n_points, p(T.bad), p(row_start), p(row_slot), p(win), len(win), p(frame), len(frame), p(r_out), p(r_seen))

        def same_points():
            gpu_points()
            n = ref_points()
            assert st.value == 0 and cnt.value == n and np.array_equal(g_out[:n], r_out[:n]) and np.array_equal(g_seen[:n], r_seen[:n])
            return n

        # 200 entries of the window's rows, re-sent with the value they hold: the delta travels, the result stays
        ek = rng.choice(win[[row_start[k + 1] > row_start[k] for k in win]], 200).astype(np.int32)
        ei = np.array([rng.integers(0, row_start[k + 1] - row_start[k]) for k in ek], np.int32)
        ev = np.ascontiguousarray(row_slot[row_start[ek] + ei], np.int32)

        def staged_points():
            assert L.ydorb_mapdb_set_row_entries(h, p(ek), p(ei), p(ev), 200) == 0
            gpu_points()

        kept = same_points()
        # the observer counter of the frame
        cap_kf = n_kf
        ls, os_ = np.array([0, len(frame)], np.int32), np.array([0, cap_kf], np.int32)
        ckf, cw, cc, cs, cb = np.zeros(cap_kf, np.int32), np.zeros(cap_kf, np.int32), np.zeros(1, np.int32), np.zeros(1, np.uint8), np.zeros(len(frame), np.uint8)
        rkf, rw, rb = np.zeros(cap_kf, np.int32), np.zeros(cap_kf, np.int32), np.zeros(len(frame), np.uint8)

        def gpu_counter():
            assert L.ydorb_mapdb_observer_counter(h, 1, p(ls), p(frame), p(os_), p(ckf), p(cw), p(cc), p(cs), p(cb)) == 0

        def ref_counter():
            return ref.localmapref_observer_counter(p(T.obs_start), p(T.obs_kf), p(T.bad), p(frame), len(frame), p(rkf), p(rw), p(rb))

        def same_counter():
            gpu_counter()
            n = ref_counter()
            assert cs[0] == 0 and cc[0] == n and np.array_equal(ckf[:n], rkf[:n]) and np.array_equal(cw[:n], rw[:n]) and np.array_equal(cb, rb)
            return n

        n_conn = same_counter()
        ts = {k: [] for k in ("points_gpu", "points_ref", "points_gpu_200_staged", "counter_gpu", "counter_ref")}
        fns = dict(points_gpu=gpu_points, points_ref=ref_points, points_gpu_200_staged=staged_points, counter_gpu=gpu_counter, counter_ref=ref_counter)
        sync_bytes = 0
        for r in range(reps + 1):
            for k, fn in fns.items():
                t0 = time.perf_counter()
                fn()
                dt = time.perf_counter() - t0
                if r:
                    ts[k].append(dt)
                if k == "points_gpu_200_staged":
                    sync_bytes = db.row_stats()["last_row_sync_bytes"]
        assert same_points() == kept and same_counter() == n_conn
        res = {k + "_ms": stat(v) for k, v in ts.items()}
        res.update(entries_walked=E, local_points=kept, frame_keyframes=n_conn, rows_load_ms=round(load_ms, 1), delta_bytes_200_entries=sync_bytes,
                   delta_bytes_nothing_staged=0, query_upload_bytes=4 * (2 * len(win) + 1 + len(frame)), query_readback_bytes=5 * cap + 4,
                   counter_upload_bytes=4 * (2 + 2 + 1 + int((frame >= 0).sum())), row_stats=db.row_stats())
        out[tag] = res

    run("map_density", d["kf_start"], d["kf_points"])
    # synthetic rows of 2 000 entries, half of them null, for the window's keyframes; the other keyframes keep their rows
    lens = np.diff(d["kf_start"].astype(np.int64))
    lens[win] = 2000
    start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    slot = np.zeros(int(start[-1]), np.int32)
    in_window = np.zeros(n_kf, bool)
    in_window[win] = True
    for k in range(n_kf):
        if in_window[k]:
            near = d["kf_points"][d["kf_start"][max(k - 15, 0)]:d["kf_start"][min(k + 16, n_kf)]]
            row = rng.choice(near, 2000).astype(np.int32)
            row[rng.permutation(2000)[:1000]] = -1
            slot[start[k]:start[k + 1]] = row
        else:
            slot[start[k]:start[k + 1]] = d["kf_points"][d["kf_start"][k]:d["kf_start"][k + 1]]
    run("rows_of_2000_half_null", start, slot)
    db.close()
    # the adapter level: tests/cpp_host/localmap_run.cpp's stand-ins (140 keyframes, 4 000 points, five frames per repetition)
    import subprocess
    exe = os.path.join(tempfile.mkdtemp(prefix="lmbench"), "localmap_run")
    lib_dir = os.path.join(ROOT, "ydorbslam_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpu_harness", "mockrt"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp_host", "localmap_run.cpp"), "-o", exe, "-L" + lib_dir, "-l:libydorb.so", "-Wl,-rpath," + lib_dir])
    r = subprocess.run([exe, str(reps)], stdout=subprocess.PIPE, text=True, check=True)
    lines = {w[0]: w[1:] for w in (ln.split() for ln in r.stdout.splitlines())}
    assert all(lines["A_%s_same" % k] == ["1"] for k in ("local_keyframes", "reference_keyframe", "local_points", "seen", "nulled"))
    out["adapter_five_frames"] = {k: [float(v) for v in lines[k]] for k in lines if k.startswith("time_")}
    return out


def bench_descriptors(reps):
    """The map-size table of --resident with a descriptor block per keyframe (one row per entry of its map-point vector) and the views of
    every point loaded once.  Then, for two point lists - the 300 points a LocalMapping pass touches and the local window's 7 750 - and
    alternating in every repetition on the same lists:
      resident   ydorb_mapdb_distinctive_descriptors with nothing staged, and with the lists' views re-staged first (staging timed apart);
      flat       the path a caller of ydorb_distinctive_descriptors must run: the host gather of every observer's row and the call.  The
                 gather here is one numpy fancy index over a flat descriptor matrix, which flatters it against the reference's walk
                 through getObservations() and each keyframe's cv::Mat;
      oracle     oracle.orb_oracle.distinctive_descriptor per point on the gathered rows, one thread (fewer repetitions).
    Results are compared exactly before timing.  Bytes uploaded per pass: the resident query sends the slots (plus the delta when views
    were staged, from ydorb_mapdb_desc_stats); the flat path sends every gathered row and the offsets."""
    from oracle import orb_oracle
    from ydorbslam_amd._lib import YdMapDbDescStats
    orb_oracle.build()
    n_kf, n_points, window = SIZES["map"]
    L = y.lib()
    d = make_map(n_kf, n_points, window)
    T = d["T"]
    rng = np.random.default_rng(7)
    n_desc = int(d["kf_start"][-1])
    base = rng.integers(0, 256, (64, 32)).astype(np.uint8)                        # near-duplicate rows, as matched descriptors are
    desc = base[rng.integers(0, 64, n_desc)]
    flips = rng.integers(0, 256, (n_desc, 3))
    for j in range(3):
        desc[np.arange(n_desc), flips[:, j] >> 3] ^= (1 << (flips[:, j] & 7)).astype(np.uint8)
    desc = np.ascontiguousarray(desc)
    # where each observation lies in its keyframe's block: kf_points is sorted by keyframe, stably, so the rank within the keyframe
    by_kf = np.argsort(T.obs_kf, kind="stable")
    view_idx = np.zeros(d["n_obs"], np.int32)
    view_idx[by_kf] = (np.arange(d["n_obs"]) - d["kf_start"][T.obs_kf[by_kf]]).astype(np.int32)
    row_of_obs = (d["kf_start"][T.obs_kf] + view_idx).astype(np.int64)             # the flat path's gather index
    out = dict(keyframes=n_kf, points=n_points, observations=d["n_obs"], descriptors=n_desc)
    h = C.c_void_p()
    y._lib.check(L.ydorb_mapdb_create(0, n_points, n_kf, 2 * d["n_obs"], C.byref(h)))
    y._lib.check(L.ydorb_mapdb_reserve_descriptors(h, 2 * d["n_obs"], 2 * n_desc))
    all_slots, kf_slots = np.arange(n_points, dtype=np.int32), np.arange(n_kf, dtype=np.int32)

    def dstats():
        st = YdMapDbDescStats()
        L.ydorb_mapdb_desc_stats(h, C.byref(st))
        return {k: int(getattr(st, k)) for k, _ in YdMapDbDescStats._fields_}

    t0 = time.perf_counter()
    assert L.ydorb_mapdb_set_centres(h, p(kf_slots), n_kf, p(d["centre"])) == 0
    assert L.ydorb_mapdb_set_points(h, p(all_slots), n_points, p(T.obs_start), p(T.obs_kf), p(T.obs_level), p(T.bad), p(d["ref_kf"]), p(d["ref_level"]), p(d["pos"])) == 0, L.ydorb_last_error()
    assert L.ydorb_mapdb_set_keyframe_descriptors(h, p(kf_slots), n_kf, p(d["kf_start"]), p(desc)) == 0, L.ydorb_last_error()
    assert L.ydorb_mapdb_set_point_views(h, p(all_slots), n_points, p(T.obs_start), p(T.obs_kf), p(view_idx)) == 0, L.ydorb_last_error()
    one = np.zeros(1, np.int32)
    o1 = [np.zeros(1, np.int32), np.zeros(2, np.int32), np.zeros(32, np.uint8), np.zeros(1, np.uint8)]
    assert L.ydorb_mapdb_distinctive_descriptors(h, p(one), 1, *[p(a) for a in o1]) == 0, L.ydorb_last_error()
    out["load_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    out["load_desc_sync_bytes"] = dstats()["last_desc_sync_bytes"]
    matcher = y.OrbMatcher()
    k0 = n_kf // 2
    wide = np.arange(k0, min(k0 + 4 * window, n_kf))
    local = np.unique(np.concatenate([d["kf_points"][d["kf_start"][k]:d["kf_start"][k + 1]] for k in wide]))[:SIZES["local"][1]].astype(np.int32)
    for label, slots in (("pass_300_points", np.ascontiguousarray(local[:300])), ("local_window_points", local)):
        n = len(slots)
        res = [np.zeros(n, np.int32), np.zeros((n, 2), np.int32), np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)]
        resident = lambda: L.ydorb_mapdb_distinctive_descriptors(h, p(slots), n, *[p(a) for a in res])
        m = np.diff(T.obs_start.astype(np.int64))[slots]
        offsets = np.concatenate([[0], np.cumsum(m)]).astype(np.int32)
        take = np.concatenate([np.arange(T.obs_start[q], T.obs_start[q + 1]) for q in slots])
        sv = [np.ascontiguousarray(a) for a in (offsets, T.obs_kf[take], view_idx[take])]
        stage = lambda: L.ydorb_mapdb_set_point_views(h, p(slots), n, *[p(a) for a in sv])
        best = np.zeros(n, np.int32)
        box = {}

        def flat():
            t = time.perf_counter()
            box["rows"] = desc[row_of_obs[take]]                                   # the host gather, 32 bytes per observation
            box["gather"] = time.perf_counter() - t
            return matcher._L.ydorb_distinctive_descriptors(matcher._h, p(box["rows"]), p(offsets), n, p(best))

        assert resident() == 0, L.ydorb_last_error()
        assert flat() == 0, L.ydorb_last_error()
        live = res[3] == 0
        assert np.array_equal(res[0][live], best[live]) and np.array_equal(res[2][live], box["rows"][offsets[:-1][live] + best[live]])
        assert (res[3][~live] == 1).all() and int((~live).sum()) == int(T.bad[slots].sum())      # the flat entry has no bad flag: a caller skips those
        want = np.array([orb_oracle.distinctive_descriptor(box["rows"][offsets[i]:offsets[i + 1]]) for i in range(n)], np.int32)
        assert np.array_equal(want, best)
        ts = dict(resident=[], stage=[], resident_after_stage=[], flat=[], gather=[], oracle=[])
        staged_bytes = 0
        for r in range(reps + 1):
            t = [time.perf_counter()]
            assert resident() == 0
            t.append(time.perf_counter())
            assert flat() == 0
            t.append(time.perf_counter())
            assert stage() == 0
            t.append(time.perf_counter())
            assert resident() == 0
            t.append(time.perf_counter())
            staged_bytes = dstats()["last_desc_sync_bytes"]
            if r:
                ts["resident"].append(t[1] - t[0]); ts["flat"].append(t[2] - t[1]); ts["gather"].append(box["gather"])
                ts["stage"].append(t[3] - t[2]); ts["resident_after_stage"].append(t[4] - t[3])
            if r and r <= max(3, reps // 5):
                u = time.perf_counter()
                for i in range(n):
                    orb_oracle.distinctive_descriptor(box["rows"][offsets[i]:offsets[i + 1]])
                ts["oracle"].append(time.perf_counter() - u)
        out[label] = dict(points=n, observations=int(offsets[-1]), resident_query_ms=stat(ts["resident"]), flat_gather_and_call_ms=stat(ts["flat"]),
                          flat_gather_alone_ms=stat(ts["gather"]), stage_views_ms=stat(ts["stage"]), resident_query_after_staging_ms=stat(ts["resident_after_stage"]),
                          cpu_oracle_ms=stat(ts["oracle"]), resident_upload_bytes=4 * n, resident_upload_bytes_after_staging=4 * n + staged_bytes,
                          flat_upload_bytes=32 * int(offsets[-1]) + 4 * (n + 1))
    L.ydorb_mapdb_destroy(h)
    return out


def flatten_times():
    """Host time of the adapters' three flattenings on stand-ins at the local size (31 keyframes, 7 750 points)."""
    m = S.random_map(5, 31, 7750, 4, 8, level_spread=1)
    scene = S.adapter_scene(m, 8.0, seed=2)
    tmp = tempfile.mkdtemp(prefix="mmbench")
    exe = S.build_adapter_exe(os.path.join(tmp, "mapmaint_run"))
    runs = [S.run_adapters(exe, tmp, scene, 0, list(range(31)), [15], S.scale_factors())["flatten_us"] for _ in range(5)]
    return {k: round(float(np.median([r[k] for r in runs])) / 1e3, 4) for k in runs[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", choices=["local", "map", "both"], default="both")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--flatten", action="store_true")
    ap.add_argument("--resident", action="store_true", help="time the resident map table (ydorb_mapdb_*) beside the flat entries instead")
    ap.add_argument("--kernel-ms", action="append", default=[], help="SIZE=MS: k_normal_depth's time from a kernel trace, for the bytes-per-second figure")
    ap.add_argument("--correct", action="store_true", help="time ydorb_mapdb_correct beside the route it replaces instead")
    ap.add_argument("--local-map", action="store_true", help="time the keyframe-row queries of updateLocalMap (DESIGN.md section 6o) beside the host restatement instead")
    ap.add_argument("--descriptors", action="store_true", help="time computeDistinctiveDescriptors on the resident descriptors (DESIGN.md section 6p) beside the flat path and the CPU oracle instead")
    a = ap.parse_args()
    if a.descriptors:
        res = bench_descriptors(a.reps)
        M.release()
        print(json.dumps(res))
        return
    if a.local_map:
        res = bench_local_map(a.reps)
        M.release()
        print(json.dumps(res))
        return
    if a.correct:
        res = bench_correct(a.reps)
        M.release()
        print(json.dumps(res))
        return
    if a.resident:
        res = bench_resident(a.reps)
        M.release()
        print(json.dumps(res))
        return
    res = {}
    for name in (["local", "map"] if a.size == "both" else [a.size]):
        res[name] = bench_size(name, a.reps)
    for kv in a.kernel_ms:
        name, ms = kv.split("=")
        if name in res:
            nd = res[name]["normal_depth"]
            nd["kernel_ms"] = float(ms)
            nd["kernel_GB_per_s"] = round(nd["algorithmic_bytes"] / (float(ms) * 1e-3) / 1e9, 1)
    if a.flatten:
        res["flatten_ms_local"] = flatten_times()
    M.release()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
