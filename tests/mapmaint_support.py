"""Test support of map maintenance: builds the CPU restatement tests/mapmaint_ref/mapmaint_ref.cpp with oracle/Makefile's compiler
flags, runs it through the product's own Python wrappers (the restatement's entries have the ABI's signatures), and makes the tables
the CPU and GPU tests share: seeded random maps, the redundancy boundaries and the comparison helpers.  Every comparison is exact."""
import ctypes as C
import os
import re
import shlex
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "mapmaint_ref", "mapmaint_ref.cpp")
_REF = None
f32 = np.float32


def _flags():
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return shlex.split(re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1))


def ref():
    global _REF
    if _REF is None:
        from ydorbslam_amd._lib import SYMBOLS
        out = os.path.join(tempfile.mkdtemp(prefix="mapref"), "libmapref.so")
        subprocess.check_call(["g++", *_flags(), "-shared", "-o", out, SRC, "-lm"])
        L = C.CDLL(out)
        for name in ("update_normal_depth", "covisibility", "keyframe_redundancy"):
            fn = getattr(L, "mapref_" + name)
            fn.restype, fn.argtypes = SYMBOLS["ydorb_map_" + name]
        L.mapref_sequential_culling.restype = C.c_int
        L.mapref_sequential_culling.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 6
        _REF = L
    return _REF


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def ref_update_normal_depth(table, pos, centre, ref_kf, ref_level, scale_factors):
    from ydorbslam_amd.map_maintenance import update_normal_depth
    return update_normal_depth(table, pos, centre, ref_kf, ref_level, scale_factors, fn=ref().mapref_update_normal_depth)


def ref_covisibility(table, query_kf, lists, capacities=None):
    from ydorbslam_amd.map_maintenance import covisibility
    return covisibility(table, query_kf, lists, capacities, fn=ref().mapref_covisibility)


def ref_keyframe_redundancy(table, cand_kf, lists, own_levels, removed=None, th_obs=3):
    from ydorbslam_amd.map_maintenance import keyframe_redundancy
    return keyframe_redundancy(table, cand_kf, lists, own_levels, removed, th_obs, fn=ref().mapref_keyframe_redundancy)


def ref_sequential_culling(table, cand_kf, lists, own_levels, th_obs=3, not_erase=None):
    """The sequential-erasure routine.  Returns dict(verdict, erased, n_counted, n_redundant [K], bad [n_points])."""
    from ydorbslam_amd.map_maintenance import _csr
    cand_kf = np.ascontiguousarray(cand_kf, np.int32)
    K = len(cand_kf)
    start, idx = _csr(lists, np.int32)
    _, own = _csr(own_levels, np.uint8)
    ne = None if not_erase is None else np.ascontiguousarray(not_erase, np.uint8)
    verdict, erased = np.zeros(max(K, 1), np.uint8), np.zeros(max(K, 1), np.uint8)
    nc, nr, bad = np.zeros(max(K, 1), np.int32), np.zeros(max(K, 1), np.int32), np.zeros(max(table.n_points, 1), np.uint8)
    ref().mapref_sequential_culling(C.byref(table.struct), _p(cand_kf), K, _p(start), _p(idx), _p(own), th_obs, _p(ne), _p(verdict), _p(erased),
                                    _p(nc), _p(nr), _p(bad))
    return dict(verdict=verdict[:K], erased=erased[:K], n_counted=nc[:K], n_redundant=nr[:K], bad=bad[:table.n_points])


def masked_culling(redundancy, table, cand_kf, lists, own_levels, th_obs=3, not_erase=None):
    """keyFrameCullingImpl's walk over `redundancy` (the product entry or the restatement): ask once, find the first candidate with cull
    at or after the cursor, mask it when it may be erased, ask again for the rest.  Returns dict(verdict, erased, n_counted, n_redundant,
    calls): each candidate's figures are those of the call that judged it."""
    K = len(cand_kf)
    removed = np.zeros(table.n_keyframes, np.uint8)
    verdict, erased = np.zeros(K, np.uint8), np.zeros(K, np.uint8)
    nc, nr = np.zeros(K, np.int32), np.zeros(K, np.int32)
    at, calls = 0, 0
    while at < K:
        r = redundancy(table, cand_kf[at:], lists[at:], own_levels[at:], removed.copy() if calls else None, th_obs)
        calls += 1
        k = 0
        while at + k < K:
            j = at + k
            verdict[j], nc[j], nr[j] = r["cull"][k], r["n_counted"][k], r["n_redundant"][k]
            k += 1
            if verdict[j] and not (not_erase is not None and not_erase[j]):
                erased[j] = 1
                removed[cand_kf[j]] = 1
                break
        at += k
    return dict(verdict=verdict, erased=erased, n_counted=nc, n_redundant=nr, calls=calls)


def scale_factors(scale_factor=1.2, n_levels=8):
    sf = np.ones(n_levels, f32)
    for i in range(1, n_levels):
        sf[i] = sf[i - 1] * f32(scale_factor)
    return sf


# ------------------------------------------------------------------------------------------------------------ tables
def random_map(seed, n_keyframes=40, n_points=600, min_obs=1, max_obs=12, stereo_share=0.5, bad_share=0.0, n_levels=8, level_spread=None):
    """A seeded map: every point is observed by min_obs .. max_obs distinct keyframes in a shuffled order, at octaves drawn around a
    per-point base octave (so that neighbouring levels are common), half of the observations stereo.  Returns dict(table, observers,
    levels, stereo, pos, centre, ref_kf, ref_level, kf_points, kf_levels): kf_points[k] / kf_levels[k] = the points keyframe k observes
    and the octaves of its own keypoints, as its map-point vector would list them."""
    from ydorbslam_amd.map_maintenance import ObservationTable
    rng = np.random.default_rng(seed)
    observers, levels, stereo = [], [], []
    for _ in range(n_points):
        m = int(rng.integers(min_obs, min(max_obs, n_keyframes) + 1))
        observers.append(rng.permutation(n_keyframes)[:m].astype(np.int32))
        base = int(rng.integers(0, n_levels))
        spread = 2 if level_spread is None else level_spread
        levels.append(np.clip(base + rng.integers(-spread, spread + 1, m), 0, n_levels - 1).astype(np.uint8))
        stereo.append((rng.uniform(size=m) < stereo_share).astype(np.uint8))
    bad = (rng.uniform(size=n_points) < bad_share).astype(np.uint8)
    table = ObservationTable(n_keyframes, observers, levels, stereo, bad)
    centre = rng.uniform(-4.0, 4.0, (n_keyframes, 3)).astype(f32)
    pos = (rng.uniform(-6.0, 6.0, (n_points, 3)) + np.array([0.0, 0.0, 12.0])).astype(f32)
    ref_at = [int(rng.integers(0, len(o))) if len(o) else 0 for o in observers]
    ref_kf = np.array([int(o[i]) if len(o) else 0 for o, i in zip(observers, ref_at)], np.int32)
    ref_level = np.array([int(l[i]) if len(l) else 0 for l, i in zip(levels, ref_at)], np.uint8)
    kf_points, kf_levels = [[] for _ in range(n_keyframes)], [[] for _ in range(n_keyframes)]
    for p, (o, l) in enumerate(zip(observers, levels)):
        for k, lv in zip(o, l):
            kf_points[k].append(p)
            kf_levels[k].append(int(lv))
    return dict(table=table, observers=observers, levels=levels, stereo=stereo, pos=pos, centre=centre, ref_kf=ref_kf, ref_level=ref_level,
                kf_points=[np.array(a, np.int32) for a in kf_points], kf_levels=[np.array(a, np.uint8) for a in kf_levels])


def culling_map(seed):
    """The issue's culling tables: 40 keyframes, 600 points, 1-12 observers, half stereo; octaves within one level of the point's base,
    so that most well-observed points are redundant for their observers and candidates are culled."""
    return random_map(seed, 40, 600, 1, 12, 0.5, level_spread=1)


CULLING_SEEDS = (3, 11)


def candidates(m):
    """Every keyframe but slot 0 (the caller omits the map's first keyframe), in slot order, with its full lists."""
    cand = np.arange(1, m["table"].n_keyframes, dtype=np.int32)
    return cand, [m["kf_points"][k] for k in cand], [m["kf_levels"][k] for k in cand]


def boundary_table():
    """The redundancy boundaries on one table of 12 keyframes.  Candidate slots 1 .. 6 each list one point (own level 2 unless noted):
       kf 1 / point 0: mono observers 1, 7, 8        weight 3 = thObs      -> counted, not redundant (3 > 3 is false)
       kf 2 / point 1: mono observers 2, 7, 8, 9     weight 4, others at level 3 = own + 1 -> redundant
       kf 3 / point 2: mono observers 3, 7, 8, 9     weight 4, others at level 4 = own + 2 -> counted, not redundant
       kf 4 / point 3: one stereo observer 4         weight 2, nothing removed -> counted (not bad), not redundant
       kf 5 / points 4 .. 13: ten points, nine redundant, one with weight 3 -> 9 of 10: 9 > 9.0 is false, not culled
       kf 6 / points 14 .. 23: ten points, all redundant -> 10 of 10: culled
    Returns (table, cand_kf, lists, own_levels, want) with want = dict(n_counted, n_redundant, cull)."""
    from ydorbslam_amd.map_maintenance import ObservationTable
    obs, lev, st = [], [], []

    def point(kfs, lvs, stereo=None):
        obs.append(kfs); lev.append(lvs); st.append(stereo or [0] * len(kfs))
        return len(obs) - 1

    lists = [[point([1, 7, 8], [2, 2, 2])], [point([2, 7, 8, 9], [2, 3, 3, 3])], [point([3, 7, 8, 9], [2, 4, 4, 4])], [point([4], [2], [1])]]
    lists.append([point([5, 7, 8, 9], [2, 2, 3, 1]) for _ in range(9)] + [point([5, 7, 8], [2, 2, 2])])
    lists.append([point([9, 6, 8, 7], [0, 2, 3, 1]) for _ in range(10)])
    table = ObservationTable(12, obs, lev, st)
    own = [[2] * len(a) for a in lists]
    want = dict(n_counted=[1, 1, 1, 1, 10, 10], n_redundant=[0, 1, 0, 0, 9, 10], cull=[0, 1, 0, 0, 0, 1])
    return table, np.arange(1, 7, dtype=np.int32), lists, own, want


def same_normal_depth(got, want):
    """Status bytes and the bit patterns of every float."""
    assert np.array_equal(got["status"], want["status"])
    for k in ("normal", "min_distance", "max_distance"):
        assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint32), np.ascontiguousarray(want[k]).view(np.uint32)), k


def same_covisibility(got, want):
    assert len(got) == len(want)
    for q, (g, w) in enumerate(zip(got, want)):
        assert g["status"] == w["status"] and g["count"] == w["count"], q
        assert np.array_equal(g["kf"], w["kf"]) and np.array_equal(g["weight"], w["weight"]), q
        assert np.array_equal(g["raw_kf"], w["raw_kf"]) and np.array_equal(g["raw_weight"], w["raw_weight"]), q   # untouched past the count


def same_redundancy(got, want):
    for k in ("n_counted", "n_redundant", "cull"):
        assert np.array_equal(got[k], want[k]), k


# ------------------------------------------------------------------------------------------------------------ adapter scenes
def adapter_scene(m, th_depth=8.0, seed=0, not_erase=()):
    """Keyframes with keypoint vectors for a random_map(): keyframe k carries its observed points at increasing keypoint indices with
    null entries between them; a keypoint's octave and stereo flag (right x >= 0) are those of the table's observation; 6 % of the depths
    lie beyond th_depth and 4 % are negative, so that the culling lists are shorter than the map-point vectors.  Returns dict(kfs,
    points, th_depth): kfs[k] = dict(centre, not_erase, octave, right_x, depth, mp), points[p] = dict(pos, bad, ref_kf, obs = [(kf, idx)])."""
    rng = np.random.default_rng(seed)
    T = m["table"]
    stereo_of = [{int(k): int(s) for k, s in zip(o, st)} for o, st in zip(m["observers"], m["stereo"])]
    kfs, idx_in = [], [dict() for _ in range(T.n_points)]
    for k in range(T.n_keyframes):
        pts, lvs = m["kf_points"][k], m["kf_levels"][k]
        n = len(pts)
        n_kp = n + n // 4 + 1
        at = np.sort(rng.permutation(n_kp)[:n])
        mp = np.full(n_kp, -1, np.int32)
        octave = rng.integers(0, 8, n_kp).astype(np.int32)
        right_x = np.full(n_kp, -1.0, f32)
        mp[at], octave[at] = pts, lvs
        for i, p in zip(at, pts):
            idx_in[p][k] = int(i)
            if stereo_of[p][k]:
                right_x[i] = 10.0
        depth = rng.uniform(0.5, 0.9 * th_depth, n_kp).astype(f32)
        u = rng.uniform(size=n_kp)
        depth[u < 0.06] = f32(1.2 * th_depth)
        depth[u > 0.96] = f32(-1.0)
        kfs.append(dict(centre=m["centre"][k], not_erase=int(k in not_erase), octave=octave, right_x=right_x, depth=depth, mp=mp))
    points = [dict(pos=m["pos"][p], bad=int(T.bad[p]), ref_kf=int(m["ref_kf"][p]), obs=[(int(k), idx_in[p][int(k)]) for k in m["observers"][p]])
              for p in range(T.n_points)]
    return dict(kfs=kfs, points=points, th_depth=float(th_depth))


def adapter_blob(scene, current, covisible, queries, sf):
    i32 = lambda *v: np.array(v, np.int32).tobytes()
    b = [i32(len(scene["kfs"]), len(scene["points"]), len(sf)), np.asarray(sf, f32).tobytes(), np.array([scene["th_depth"]], f32).tobytes(),
         i32(current), i32(len(covisible)), i32(*covisible), i32(len(queries)), i32(*queries)]
    for k in scene["kfs"]:
        b += [np.asarray(k["centre"], f32).tobytes(), i32(k["not_erase"], len(k["mp"])), k["octave"].astype(np.int32).tobytes(),
              k["right_x"].astype(f32).tobytes(), k["depth"].astype(f32).tobytes(), k["mp"].astype(np.int32).tobytes()]
    for p in scene["points"]:
        b += [np.asarray(p["pos"], f32).tobytes(), i32(p["bad"], p["ref_kf"], len(p["obs"])), np.array(p["obs"], np.int32).reshape(-1).tobytes()]
    return b"".join(b)


def build_adapter_exe(out):
    lib_dir = os.path.join(ROOT, "ydorbslam_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpu_harness", "mockrt"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp_host", "mapmaint_run.cpp"), "-o", out,
                           "-L" + lib_dir, "-l:libydorb.so", "-Wl,-rpath," + lib_dir])
    return out


def run_adapters(exe, tmp, scene, current, covisible, queries, sf):
    """Runs tests/cpp_host/mapmaint_run.cpp.  Returns dict(order [per point: keyframe ids in the container's order], applied, normal,
    min_distance, max_distance, counters [per query: {kf: weight}], flagged, bad [n_kf], flatten_us {name: microseconds})."""
    inp, outp = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    open(inp, "wb").write(adapter_blob(scene, current, covisible, queries, sf))
    r = subprocess.run([exe, inp, outp], stdout=subprocess.PIPE, text=True, check=True)
    raw = np.frombuffer(open(outp, "rb").read(), np.int32)
    at, order = 0, []
    for _ in scene["points"]:
        n = int(raw[at])
        order.append(raw[at + 1:at + 1 + n].copy())
        at += 1 + n
    n_pts, n_kf = len(scene["points"]), len(scene["kfs"])
    rec = raw[at:at + 6 * n_pts].reshape(n_pts, 6)
    at += 6 * n_pts
    counters = []
    for _ in queries:
        n = int(raw[at])
        pairs = raw[at + 1:at + 1 + 2 * n].reshape(n, 2)
        counters.append({int(k): int(w) for k, w in pairs})
        at += 1 + 2 * n
    n = int(raw[at])
    flagged = raw[at + 1:at + 1 + n].tolist()
    at += 1 + n
    bad = raw[at:at + n_kf].copy()
    assert at + n_kf == len(raw)
    us = {ln.split()[0][len("flatten_"):-len("_us")]: float(ln.split()[1]) for ln in r.stdout.splitlines() if ln.startswith("flatten_")}
    return dict(order=order, applied=rec[:, 0].copy(), normal=np.ascontiguousarray(rec[:, 1:4]).view(f32), min_distance=np.ascontiguousarray(rec[:, 4]).view(f32),
                max_distance=np.ascontiguousarray(rec[:, 5]).view(f32), counters=counters, flagged=flagged, bad=bad, flatten_us=us)


def scene_table(scene, order):
    """The table the adapters flatten when the observation containers iterate in `order`, over keyframe slots = ids and all points.
    Returns (table, ref_level)."""
    from ydorbslam_amd.map_maintenance import ObservationTable
    kfs, idx = scene["kfs"], [dict(p["obs"]) for p in scene["points"]]
    lev = [[int(kfs[k]["octave"][idx[p][int(k)]]) for k in o] for p, o in enumerate(order)]
    st = [[int(kfs[k]["right_x"][idx[p][int(k)]] >= 0) for k in o] for p, o in enumerate(order)]
    T = ObservationTable(len(kfs), [np.asarray(o, np.int32) for o in order], lev, st, [p["bad"] for p in scene["points"]])
    ref_level = [int(kfs[p["ref_kf"]]["octave"][idx[i].get(p["ref_kf"], 0)]) if p["obs"] else 0 for i, p in enumerate(scene["points"])]
    return T, np.array(ref_level, np.uint8)


def scene_lists(scene, kf_ids, depth_test):
    """Per keyframe the non-null map-point entries in keypoint order (those passing !(depth > thDepth || depth < 0) when depth_test) and
    the octaves of its own keypoints."""
    lists, own = [], []
    for k in kf_ids:
        K = scene["kfs"][k]
        keep = K["mp"] >= 0
        if depth_test:
            keep &= ~((K["depth"] > f32(scene["th_depth"])) | (K["depth"] < 0))
        lists.append(K["mp"][keep].astype(np.int32))
        own.append(K["octave"][keep].astype(np.uint8))
    return lists, own
