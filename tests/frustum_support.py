"""Test support of Tracking::searchLocalPoints' geometry: builds the CPU restatement tests/frustum_ref/frustum_ref.cpp with
oracle/Makefile's compiler flags, the level tables (from the restatement library's log, never numpy's), hand-built rows, the batch scene
of the GPU parity tests and the frame + local map of the fused-search tests."""
import ctypes as C
import functools
import os
import re
import shlex
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "frustum_ref", "frustum_ref.cpp")
_REF = None

K = (520.0, 515.0, 320.0, 240.0)
BF = float(np.float32(0.12) * np.float32(K[0]))
BOUNDS = (0.0, 640.0, 0.0, 480.0)
f32 = np.float32


def _flags():
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return shlex.split(re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1))


def ref():
    global _REF
    if _REF is None:
        out = os.path.join(tempfile.mkdtemp(prefix="frustumref"), "libfrustumref.so")
        # the adapter header (for its table builder) includes <opencv2/core.hpp>: the declaration-only mock serves, nothing of it is called
        subprocess.check_call(["g++", *_flags(), "-I" + os.path.join(ROOT, "tests", "cpu_harness", "mock"), "-shared", "-o", out, SRC, "-lm"])
        L = C.CDLL(out)
        L.frustumref_cull.restype = C.c_int
        L.frustumref_cull.argtypes = [C.c_void_p] * 5
        L.frustumref_predict_level.restype = C.c_int
        L.frustumref_predict_level.argtypes = [C.c_float, C.c_float, C.c_int]
        L.frustumref_predict_levels.restype = None
        L.frustumref_predict_levels.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p]
        L.frustumref_level_ratio_table.restype = None
        L.frustumref_level_ratio_table.argtypes = [C.c_float, C.c_int, C.c_void_p]
        L.frustumref_logf.restype = C.c_float
        L.frustumref_logf.argtypes = [C.c_float]
        _REF = L
    return _REF


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@functools.lru_cache(maxsize=None)
def _levels(scale_factor, n_levels):
    logsf = f32(ref().frustumref_logf(C.c_float(scale_factor)))
    t = np.zeros(max(n_levels - 1, 1), f32)
    ref().frustumref_level_ratio_table(C.c_float(logsf), n_levels, _p(t))
    return logsf, t[:n_levels - 1]


def log_scale_factor(scale_factor=1.2):
    """m_flt_logScaleFactor = log(m_flt_scaleFactor) in float, by the C library the restatement links."""
    return _levels(float(scale_factor), 8)[0]


def level_table(scale_factor=1.2, n_levels=8):
    """The adapter's levelRatioTable for this scale factor: [n_levels - 1] float32."""
    return _levels(float(scale_factor), int(n_levels))[1].copy()


def formula_levels(ratio, scale_factor, n_levels):
    ratio = np.ascontiguousarray(ratio, f32)
    out = np.zeros(len(ratio), np.int32)
    ref().frustumref_predict_levels(_p(ratio), len(ratio), C.c_float(log_scale_factor(scale_factor)), n_levels, _p(out))
    return out


def table_levels(ratio, table):
    """The device's rule: the number of table entries strictly below the ratio."""
    return (np.asarray(table, f32)[None, :] < np.asarray(ratio, f32)[:, None]).sum(axis=1).astype(np.int32)


def scale_factors(scale_factor=1.2, n_levels=8):
    sf = np.ones(n_levels, f32)
    for i in range(1, n_levels):
        sf[i] = sf[i - 1] * f32(scale_factor)
    return sf


# ------------------------------------------------------------------------------------------------------------ geometry helpers
def rot(axis, angle):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    S = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * S + (1 - np.cos(angle)) * S @ S


def pose(R=np.eye(3), centre=(0, 0, 0)):
    """(Tcw 3x4 float32, Ow float32) of a camera with rotation Rcw = R and centre `centre`."""
    R = np.asarray(R, np.float64)
    return np.hstack([R, (-R @ np.asarray(centre, np.float64))[:, None]]).astype(f32), np.asarray(centre, f32)


def view(T, Ow, scale_factor=1.2, n_levels=8, cos_limit=0.5):
    """(YdFrustumView, its frame's m_flt_logScaleFactor)."""
    from ydorbslam_amd.frustum import make_view
    return make_view(T, Ow, K, BF, BOUNDS, level_table(scale_factor, n_levels), scale_factors(scale_factor, n_levels), cos_limit), \
        log_scale_factor(scale_factor)


def ref_cull(views, logs, table, lists, skips):
    """The restatement on the arguments of ydorbslam_amd.frustum.frustum_cull (logs[f] = view f's m_flt_logScaleFactor); same return value."""
    from ydorbslam_amd.frustum import FrustumBatch
    B = FrustumBatch(views, table, lists, skips)
    rows, status, n_in = B.outputs()
    lg = np.ascontiguousarray(list(logs) + [0], f32)
    ref().frustumref_cull(C.byref(B.struct), _p(lg), _p(rows), _p(status), _p(n_in))
    return B.split(rows, status, n_in)


def ref_queries(rows, status, has_obs, th, sf):
    """The query build of searchByProjectionInFrameAndMapPoint, one map point after the other as the adapter's host loop writes it."""
    from ydorbslam_amd import QUERY_DTYPE
    q = np.zeros(len(rows), QUERY_DTYPE)
    for i in range(len(rows)):
        if status[i] != 0:
            continue
        lvl = int(rows["level"][i])
        radius = f32(th) * (f32(2.5) if float(rows["view_cos"][i]) > 0.998 else f32(4.0))
        r = f32(radius * sf[lvl])
        q[i] = (rows["u"][i], rows["v"][i], r, lvl - 1, lvl, rows["ur"][i], r, 0.0, lvl, 1 | (2 if has_obs[i] else 0))
    return q


def queries_from_rows(rows, status, has_observations, th, scale_factors):
    """The query build of searchByProjectionInFrameAndMapPoint (orbMatcher.cpp:28-38) on isInCameraFrustum's rows, vectorised: the host
    step of the composition that ydorb_search_local_points is defined by (ref_queries is the same build written row by row)."""
    from ydorbslam_amd import QUERY_DTYPE
    q = np.zeros(len(rows), QUERY_DTYPE)
    ok = np.asarray(status) == 0
    sf = np.asarray(scale_factors, f32)
    radius = f32(th) * np.where(rows["view_cos"].astype(np.float64) > 0.998, f32(2.5), f32(4.0)).astype(f32)
    r = (radius * sf[np.clip(rows["level"], 0, len(sf) - 1)]).astype(f32)
    for k in ("u", "v", "ur"):
        q[k][ok] = rows[k][ok]
    q["r"][ok] = q["rs"][ok] = r[ok]
    q["min_level"][ok], q["max_level"][ok], q["level"][ok] = rows["level"][ok] - 1, rows["level"][ok], rows["level"][ok]
    q["flags"][ok] = 1 | np.where(np.asarray(has_observations)[ok] != 0, 2, 0)
    return q


def search_local_points_composed(matcher, frame, view, table, skip, has_observations, th, taken=None, assigned=None):
    """What ydorb_search_local_points is defined as, in three steps through the ABI: ydorb_frustum_cull with one view over all points,
    the query build on the host, ydorb_search_by_projection (mode 0; skipped when no point is in view).  `matcher` was created with
    check_orientation=False.  Returns the dict of ydorbslam_amd.frustum.search_local_points."""
    from ydorbslam_amd.frustum import frustum_cull
    r = frustum_cull([view], table, [np.arange(table.n, dtype=np.int32)], [skip])[0]
    taken = np.zeros(frame.n, np.uint8) if taken is None else np.ascontiguousarray(taken, np.uint8).copy()
    assigned = np.full(frame.n, -1, np.int32) if assigned is None else np.ascontiguousarray(assigned, np.int32).copy()
    n = 0
    if r["n_in_view"] > 0:
        q = queries_from_rows(r["rows"], r["status"], has_observations, th, np.array(view.scale_factors[:view.n_levels], f32))
        n, assigned, taken = matcher.search_by_projection(0, frame, q, table.desc, taken, assigned)
    return dict(n_to_match=r["n_in_view"], n_matches=n, assigned=assigned, taken=taken, rows=r["rows"], status=r["status"])


def same_rows(got, want):
    """Status bytes and the bit patterns of every YdTrackView field."""
    assert np.array_equal(got["status"], want["status"])
    for k in ("u", "v", "ur", "view_cos"):
        assert np.array_equal(got["rows"][k].view(np.uint32), want["rows"][k].view(np.uint32)), k
    assert np.array_equal(got["rows"]["level"], want["rows"]["level"])


# ------------------------------------------------------------------------------------------------------------ hand-built rows
def hand_rows():
    """name -> dict(P, Pn, min, max, maxd, skip, Ow, status, level, nan): one map point each in front of a camera at the world origin
    that looks down +z (Ow overridden where a row needs a stale one).  `nan` = the fields that must be NaN, `level` = the predicted
    level of an in-view row (None: not checked here)."""
    r = {}

    def row(name, P, status, Pn=None, mn=1.6, mx=9.6, maxd=8.0, skip=0, Ow=(0, 0, 0), level=None, nan=()):
        P = np.asarray(P, np.float64)
        if Pn is None:
            d = P - np.asarray(Ow, np.float64)
            Pn = d / np.linalg.norm(d) if np.isfinite(d).all() and np.linalg.norm(d) > 0 else np.array([0.0, 0.0, 1.0])
        r[name] = dict(P=P, Pn=np.asarray(Pn, np.float64), min=mn, max=mx, maxd=maxd, skip=skip, Ow=Ow, status=status, level=level, nan=nan)

    row("in_view", (0.2, 0.1, 4.0), 0, level=4)           # dist 4.006..: ratio 1.997, 1.2^3 = 1.728 < ratio <= 1.2^4 = 2.0736
    row("skipped", (0.2, 0.1, 4.0), 1, skip=1)
    row("behind", (0.2, 0.1, -4.0), 2)
    row("out_u", (10.0, 0.0, 4.0), 3)
    row("out_v", (0.0, 10.0, 4.0), 4)
    row("too_far", (0.2, 0.1, 4.0), 5, mn=0.4, mx=2.4, maxd=2.0)
    row("too_near", (0.2, 0.1, 4.0), 5, mn=8.0, mx=48.0, maxd=40.0)
    row("view_angle", (0.0, 0.1, 4.0), 6, Pn=(1.0, 0.0, 0.0))
    row("clamp_low", (0.0, 0.0, 9.0), 0, level=0)          # ratio 8 / 9 < 1: log < 0, clamped to level 0
    row("clamp_high", (0.0, 0.0, 1.7), 0, level=7)         # ratio 4.7 > 1.2^7 = 3.58: clamped to nLevels - 1
    row("pcz_zero_inf", (1.0, 0.0, 0.0), 3, mn=0.0)        # invz = inf, u = +inf: u > maxX is true, literally
    row("pcz_zero_nan", (0.0, 0.0, 0.0), 0, mn=0.0, Ow=(0, 0, -3.0), level=6, nan=("u", "v", "ur"))   # 0 * inf = NaN fails no bounds test
    row("nan_position", (np.nan, 0.0, 4.0), 0, level=0, nan=("u", "v", "ur", "view_cos"))               # NaN passes every exit; ratio NaN -> 0
    row("dist_zero", (0.0, 0.0, 0.0), 0, mn=0.0, level=7, nan=("u", "v", "ur", "view_cos"))             # ratio = 8 / 0 = inf -> nLevels - 1
    return r


def hand_batch():
    """The hand-built rows as one batch: one view and a one-entry list per row (a row may need its own Ow).  Returns (views, logs, table,
    lists, skips, names)."""
    from ydorbslam_amd.frustum import PointTable
    rows = hand_rows()
    names = sorted(rows)
    T, _ = pose()
    vl = [view(T, np.asarray(rows[n]["Ow"], f32)) for n in names]
    table = PointTable([rows[n]["P"] for n in names], [rows[n]["Pn"] for n in names], [rows[n]["min"] for n in names],
                       [rows[n]["max"] for n in names], [rows[n]["maxd"] for n in names])
    return [v for v, _ in vl], [l for _, l in vl], table, [[i] for i in range(len(names))], [[rows[n]["skip"]] for n in names], names


# ------------------------------------------------------------------------------------------------------------ batch scene
def scene(seed=5, n=300):
    """Three frames over one table of n map points around them: points in front, behind and beside the cameras; normals within ~75 degrees
    of the direction from the first camera; maximum distances that put the ratio between 1.2^-2 and 1.2^10, so that both distance
    bounds fire and every level 0-7 is predicted.  View 0 tests all points in a shuffled order, view 1 none, view 2 an overlapping
    list of n / 2 entries with repeats; 6 % of the entries carry the skip flag.  Returns (views, logs, table, lists, skips)."""
    from ydorbslam_amd.frustum import PointTable
    rng = np.random.default_rng(seed)
    poses = [pose(), pose(rot((0.1, 1, 0.05), np.radians(12.0)), (0.4, 0.05, -0.2)), pose(rot((0, 1, 0.2), np.radians(-9.0)), (-0.3, 0.0, 0.3))]
    z = rng.uniform(1.0, 12.0, n)
    P = np.stack([rng.uniform(-0.9, 0.9, n) * z, rng.uniform(-0.7, 0.7, n) * z, z], axis=1)
    P[rng.uniform(size=n) < 0.08, 2] *= -1
    d0 = np.linalg.norm(P, axis=1)
    tilt = rng.normal(size=(n, 3))
    Pn = P / d0[:, None] + 0.55 * tilt / np.linalg.norm(tilt, axis=1)[:, None] * rng.uniform(0, 2.2, n)[:, None]
    Pn /= np.linalg.norm(Pn, axis=1)[:, None]
    maxd = (d0 * 1.2 ** rng.uniform(-2.0, 10.0, n)).astype(f32)
    mind = (maxd / scale_factors()[7]).astype(f32)
    table = PointTable(P, Pn, f32(0.8) * mind, f32(1.2) * maxd, maxd)
    lists = [rng.permutation(n), np.zeros(0, np.int64), rng.integers(0, n, n // 2)]
    skips = [(rng.uniform(size=len(a)) < 0.06).astype(np.uint8) for a in lists]
    vl = [view(*p) for p in poses]
    return [v for v, _ in vl], [l for _, l in vl], table, lists, skips


# ------------------------------------------------------------------------------------------------------------ frame + local map
def local_map(seed=9, n_kp=500, n_mp=300, th=3.0):
    """One frame of n_kp keypoints and a local map of n_mp points for a search with radius factor th.  Four in five points come from
    one of 180 (of 500) of the frame's keypoints (so several points want the same keypoint), placed where the reference's getKeyPointsInArea
    (frame.cpp:337-361, restated literally by the oracle and the kernels) can return that keypoint: it keeps a feature of the window's
    cells whose x distance is GREATER than r and whose y distance is below r, and whose octave is at least the predicted level.  So the
    point is unprojected from a pixel r + 0.5 .. r + 6 beside the keypoint, a pixel of noise in y, at a random depth, with the
    keypoint's descriptor and a few bits flipped, and a maximum distance that predicts the keypoint's octave or the one below.  The
    normal is 16 degrees off the viewing ray (radius factor 4), for one point in five 1 degree (viewCos > 0.998: factor 2.5).  The
    rest lie anywhere.  Some keypoints are stereo, some already hold a point (taken), 4 % of the points are skip-flagged, one in six
    has no observations.  Returns dict(frame kps / desc / right_x, view, log, table, skip, has_obs, taken)."""
    from ydorbslam_amd import KP_DTYPE
    from ydorbslam_amd.frustum import PointTable
    rng = np.random.default_rng(seed)
    T, Ow = pose(rot((0.2, 1, 0.1), np.radians(7.0)), (0.3, -0.1, 0.2))
    R, t = T[:, :3].astype(np.float64), T[:, 3].astype(np.float64)
    sf = scale_factors().astype(np.float64)
    kps = np.zeros(n_kp, KP_DTYPE)
    kps["x"], kps["y"] = rng.uniform(20, 620, n_kp), rng.uniform(20, 460, n_kp)
    kps["octave"], kps["size"], kps["angle"], kps["class_id"] = rng.integers(0, 8, n_kp), 31, rng.uniform(0, 360, n_kp), -1
    desc = rng.integers(0, 256, (n_kp, 32), dtype=np.uint8)
    right_x = np.full(n_kp, -1.0, f32)
    pool = rng.permutation(n_kp)[:180 * n_kp // 500]
    P, Pn, maxd, mdesc = np.zeros((n_mp, 3)), np.zeros((n_mp, 3)), np.zeros(n_mp), np.zeros((n_mp, 32), np.uint8)
    for i in range(n_mp):
        tilt = 0.02 if rng.uniform() < 0.2 else 0.3
        if rng.uniform() < 0.8:
            j = int(pool[rng.integers(0, len(pool))])
            z = rng.uniform(1.5, 9.0)
            lvl = max(int(kps["octave"][j]) - int(rng.uniform() < 0.3), 0)
            r = th * (2.5 if tilt < 0.1 else 4.0) * sf[lvl]
            side = 1.0 if rng.uniform() < 0.5 else -1.0
            uv = np.array([kps["x"][j] - side * (r + rng.uniform(0.5, 6.0)), kps["y"][j] + rng.normal(0, 1.0)], np.float64)
            Xc = np.array([(uv[0] - K[2]) * z / K[0], (uv[1] - K[3]) * z / K[1], z])
            P[i] = R.T @ (Xc - t)
            if right_x[j] < 0 and rng.uniform() < 0.5:
                right_x[j] = uv[0] - BF / z
            mdesc[i] = desc[j]
            for bit in rng.integers(0, 256, int(rng.integers(0, 12))):
                mdesc[i, bit // 8] ^= np.uint8(1 << (bit % 8))
            maxd[i] = np.linalg.norm(P[i] - Ow) * 1.2 ** (lvl - 0.5)
        else:
            z = rng.uniform(-3.0, 12.0)
            P[i] = R.T @ (np.array([rng.uniform(-1.2, 1.2) * z, rng.uniform(-0.9, 0.9) * z, z]) - t)
            mdesc[i] = rng.integers(0, 256, 32, dtype=np.uint8)
            maxd[i] = np.linalg.norm(P[i] - Ow) * 1.2 ** rng.uniform(-1.0, 8.0)
        d = (P[i] - Ow) / np.linalg.norm(P[i] - Ow)
        side_dir = rng.normal(size=3)
        side_dir -= (side_dir @ d) * d                         # perpendicular to the ray: viewCos = 1 / sqrt(1 + tilt^2)
        Pn[i] = d + tilt * side_dir / np.linalg.norm(side_dir)
        Pn[i] /= np.linalg.norm(Pn[i])
    maxd = maxd.astype(f32)
    mind = (maxd / scale_factors()[7]).astype(f32)
    table = PointTable(P, Pn, f32(0.8) * mind, f32(1.2) * maxd, maxd, mdesc)
    v, lg = view(T, Ow)
    return dict(kps=kps, desc=desc, right_x=right_x, view=v, log=lg, table=table, skip=(rng.uniform(size=n_mp) < 0.04).astype(np.uint8),
                has_obs=(rng.uniform(size=n_mp) < 5 / 6).astype(np.uint8), taken=(rng.uniform(size=n_kp) < 0.05).astype(np.uint8))


def ref_search_local_points(s, th, ratio, skip=None, taken=None, assigned=None):
    """The restatement followed by the matcher oracle (oracle/matcher_oracle.cpp) on a local_map() scenario: the same dict as
    ydorbslam_amd.frustum.search_local_points, plus the queries."""
    from oracle.orb_oracle import FrameOracle
    skip = s["skip"] if skip is None else skip
    n = s["table"].n
    r = ref_cull([s["view"]], [s["log"]], s["table"], [np.arange(n)], [skip])[0]
    q = ref_queries(r["rows"], r["status"], s["has_obs"], th, scale_factors())
    taken = (s["taken"] if taken is None else taken).copy()
    assigned = np.full(len(s["kps"]), -1, np.int32) if assigned is None else assigned.copy()
    nm = 0
    if r["n_in_view"] > 0:
        fo = FrameOracle(s["kps"], s["desc"], BOUNDS, s["right_x"])
        nm, assigned, taken = fo.search_by_projection(0, q, s["table"].desc, ratio, False, taken, assigned)
    return dict(n_to_match=r["n_in_view"], n_matches=nm, assigned=assigned, taken=taken, rows=r["rows"], status=r["status"], queries=q)
