"""Scenarios, independent statements and bookkeeping replays for the matcher adapter bodies that tests/cpp_host/matcher_adapters_run.cpp
executes: searchByProjectionInFrameAndMapPoint, searchByProjectionInKeyFrameAndCurrentFrame, searchByProjectionInSim, searchBySim3, the
flat fuseByProjection / fuseBySim3 and the flat searchForTriangulation of include/ydorb/orbMatcher.hpp.

Each `statement_*` gives the flat problem an adapter has to hand to the C ABI (QUERY_DTYPE rows, query descriptors, masks) from the
scenario arrays, following DESIGN.md section 2 "Fuse search on the resident table", SURVEY.md:287-292 and the header comments of
orbMatcher.hpp, in float32, one rounded operation at a time, in the arithmetic the mock cv::Mat documents: a float gemm accumulates
rounded products in ascending k, cv::norm and Mat::dot work in double, u = fx * x / z + cx is a multiply, a divide and an add.  Each
`double_*` is the plain float64 evaluation of the same float32 inputs.  Each `expected_*` pushes the flat problem through a search
back-end (the serial oracle on the CPU, the ctypes mirror on the GPU) and replays the adapter's bookkeeping in plain Python into the
object state the host program dumps.

Scenarios are seeded and small: at most 400 features per frame or keyframe, at most 300 map points, 8 levels at 1.2, bounds 0..640 x
0..480.  A feature meant to be found ("twin") sits where Frame::getKeyPointsInArea as written keeps it, |dx| > r && |dy| < r
(frame.cpp:353), at a level its level rule as written keeps (a lower bound only: octave >= max(minLevel, maxLevel), frame.cpp:347)."""
import os
import struct
import subprocess

import numpy as np

from helpers import QUERY_DTYPE, bow_nodes, feature_vector
from oracle.orb_oracle import KP_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp_host", "matcher_adapters_run.cpp")
F32, F64 = np.float32, np.float64
W, H = 640, 480
BOUNDS = (0.0, float(W), 0.0, float(H))
FX, FY, CX, CY, BASE, BF = F32(500.0), F32(500.0), F32(319.5), F32(239.5), F32(0.08), F32(40.0)
SF = np.ones(8, F32)
for _l in range(1, 8):
    SF[_l] = SF[_l - 1] * F32(1.2)
LOG_SF = F32(np.log(F64(F32(1.2))))
INV_S2 = (F32(1.0) / (SF * SF)).astype(F32)
EPS = 2.0 ** -24


# ---- the host program ---------------------------------------------------------------------------------------------------------------
def build_program(tmp):
    exe = os.path.join(tmp, "matcher_adapters_run")
    lib_dir = os.path.join(ROOT, "ydorbslam_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpu_harness", "mockrt"),
                           "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe, "-L" + lib_dir, "-l:libydorb.so", "-Wl,-rpath," + lib_dir])
    return exe


def run_program(exe, what, blob, tmp, tag=""):
    inp, out = os.path.join(tmp, what + tag + ".in"), os.path.join(tmp, what + tag + ".out")
    open(inp, "wb").write(blob)
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(__import__("torch").__file__), "lib") + ":" + env.get("LD_LIBRARY_PATH", "")
    subprocess.check_call([exe, what, inp, out], env=env)
    return open(out, "rb").read()


# ---- float32 arithmetic of the mock cv::Mat, vectorised over points -----------------------------------------------------------------------
def gemv32(R, P):
    """R [3,3] times every row of P [N,3]: products rounded to float, accumulated in float in ascending k."""
    R, P = np.asarray(R, F32), np.asarray(P, F32).reshape(-1, 3)
    out = np.empty_like(P)
    for i in range(3):
        acc = R[i, 0] * P[:, 0]
        acc = acc + R[i, 1] * P[:, 1]
        out[:, i] = acc + R[i, 2] * P[:, 2]
    return out


def pixel32(Pc):
    with np.errstate(all="ignore"):
        x, y, z = Pc[:, 0], Pc[:, 1], Pc[:, 2]
        return (FX * x) / z + CX, (FY * y) / z + CY, z


def norm32(D):
    D = np.asarray(D, F32).astype(F64)
    return np.sqrt(D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1] + D[:, 2] * D[:, 2]).astype(F32)


def level32(max_d, dist):
    """MapPoint::predictScaleLevel: ceil(log(maxDistance / dist) / logScaleFactor) in float, clamped to 0 .. 7."""
    with np.errstate(all="ignore"):
        ratio = np.asarray(max_d, F32) / np.asarray(dist, F32)
        q = np.ceil(np.log(ratio.astype(F64)).astype(F32) / LOG_SF)
    return np.where(~(q >= 0), 0, np.where(q >= 8, 7, q)).astype(np.int32)


def in_image(u, v):
    return (u >= F32(0)) & (u < F32(W)) & (v >= F32(0)) & (v < F32(H))


def rot(axis, deg):
    a = np.asarray(axis, F64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def flip_bits(desc, n, rng, first_byte=0):
    d = np.array(desc, np.uint8)
    for b in rng.choice(np.arange(first_byte * 8, 256), int(n), replace=False):
        d[b // 8] ^= np.uint8(1 << (b % 8))
    return d


# ---- scenario storage ---------------------------------------------------------------------------------------------------------------------
class Feats:
    """The features of one frame or keyframe while a scenario is built."""

    def __init__(self):
        self.rows, self.desc = [], []

    def add(self, x, y, octave, desc, right=-1.0, angle=0.0, mp=-1):
        self.rows.append((F32(x), F32(y), int(octave), F32(angle), F32(right), int(mp)))
        self.desc.append(np.array(desc, np.uint8))
        return len(self.rows) - 1

    def __len__(self):
        return len(self.rows)

    def view(self):
        n = len(self.rows)
        kps = np.zeros(n, KP_DTYPE)
        kps["x"], kps["y"] = [r[0] for r in self.rows], [r[1] for r in self.rows]
        kps["octave"], kps["angle"] = [r[2] for r in self.rows], [r[3] for r in self.rows]
        kps["size"], kps["response"], kps["class_id"] = 31.0, 1.0, -1
        return dict(kps=kps, desc=np.array(self.desc, np.uint8).reshape(n, 32), right=np.array([r[4] for r in self.rows], F32),
                    mp_of=np.array([r[5] for r in self.rows], np.int32))


class Scene:
    """The world the host program reads: map points, keyframes, observations, one frame."""

    def __init__(self, n_points, rng):
        n = n_points
        self.n = n
        self.pos, self.normal = np.zeros((n, 3), F32), np.zeros((n, 3), F32)
        self.min_d, self.max_d = np.ones(n, F32), np.ones(n, F32)
        self.track = np.zeros((n, 4), F32)                        # projX, projY, projRightX, viewCos
        self.bad, self.in_view, self.track_level = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        self.desc = rng.integers(0, 256, (n, 32)).astype(np.uint8)
        self.obs = [dict() for _ in range(n)]                     # keyframe index -> feature index
        self.kfs = []
        self.frame = dict(T=np.eye(4, dtype=F32), **Feats().view())
        self.args = {}

    def add_keyframe(self, R, t, feats):
        R, t = np.asarray(R, F32), np.asarray(t, F32)
        kf = dict(R=R, t=t, O=gemv32(-(R.T), t)[0], **feats.view())   # the centre as the keyframe stores it, -R^T t
        kf["fv"] = feature_vector(bow_nodes(kf["desc"], 4)) if len(kf["kps"]) else (np.zeros(0, np.uint32), np.zeros(1, np.int32), np.zeros(0, np.int32))
        self.kfs.append(kf)
        return len(self.kfs) - 1

    def link(self):
        """Every keyframe slot that holds a point is one of that point's observations."""
        for k, kf in enumerate(self.kfs):
            for i, p in enumerate(kf["mp_of"]):
                if p >= 0:
                    self.obs[p][k] = i

    def world_blob(self):
        b = np.array([FX, FY, CX, CY, BASE, BF, *BOUNDS], F32).tobytes() + SF.tobytes() + struct.pack("<f", LOG_SF)
        b += struct.pack("<i", self.n)
        for i in range(self.n):
            b += self.pos[i].tobytes() + self.normal[i].tobytes() + struct.pack("<2f", self.min_d[i], self.max_d[i]) + self.track[i].tobytes()
            b += struct.pack("<3i", int(self.bad[i]), int(self.in_view[i]), int(self.track_level[i])) + self.desc[i].tobytes()
        b += struct.pack("<i", len(self.kfs))
        for kf in self.kfs:
            b += kf["R"].tobytes() + kf["t"].tobytes() + kf["O"].tobytes() + struct.pack("<i", len(kf["kps"]))
            b += kf["kps"].tobytes() + kf["desc"].tobytes() + kf["right"].tobytes() + kf["mp_of"].tobytes()
            ids, start, feat = kf["fv"]
            b += struct.pack("<i", len(ids))
            for i in range(len(ids)):
                f = np.asarray(feat[start[i]:start[i + 1]], np.uint32)
                b += struct.pack("<Ii", int(ids[i]), len(f)) + f.tobytes()
        for i in range(self.n):
            b += struct.pack("<i", len(self.obs[i])) + b"".join(struct.pack("<2i", k, idx) for k, idx in sorted(self.obs[i].items()))
        f = self.frame
        b += f["T"].astype(F32).tobytes() + struct.pack("<i", len(f["kps"])) + f["kps"].tobytes() + f["desc"].tobytes() + f["right"].tobytes() + f["mp_of"].tobytes()
        return b


def point_list_blob(idx):
    return struct.pack("<i", len(idx)) + np.asarray(idx, np.int32).tobytes()


class State:
    """The mutable object state, with the stand-ins' addObservation / addMapPoint / beReplacedBy (MapPoint::replace without the
    survivor's descriptor refresh): what a replay leaves here is what the host program must dump."""

    def __init__(self, scene):
        self.bad = [int(b) for b in scene.bad]
        self.replaced = [-1] * scene.n
        self.obs = [dict(o) for o in scene.obs]
        self.kf_mps = [[int(p) for p in kf["mp_of"]] for kf in scene.kfs]

    def n_obs(self, p):
        return len(self.obs[p])

    def add(self, p, k, idx):
        if k not in self.obs[p]:
            self.obs[p][k] = idx
        self.kf_mps[k][idx] = p

    def replace(self, p, by):
        if p == by:
            return
        held = self.obs[p]
        self.obs[p] = {}
        self.bad[p], self.replaced[p] = 1, by
        for k, idx in held.items():
            if k not in self.obs[by]:
                self.kf_mps[k][idx] = by
                self.obs[by][k] = idx
            else:
                self.kf_mps[k][idx] = -1

    def dump(self):
        return ([(self.bad[p], self.replaced[p], sorted(self.obs[p].items())) for p in range(len(self.bad))], self.kf_mps)


def parse_output(out, scene):
    ret, nvec = struct.unpack_from("<2i", out, 0)
    vec = np.frombuffer(out, np.int32, nvec, 8)
    off = 8 + 4 * nvec
    points = []
    for _ in range(scene.n):
        bad, rep, nob = struct.unpack_from("<3i", out, off); off += 12
        ob = np.frombuffer(out, np.int32, 2 * nob, off).reshape(-1, 2); off += 8 * nob
        points.append((bad, rep, [tuple(o) for o in ob.tolist()]))
    kfs = []
    for _ in scene.kfs:
        n = struct.unpack_from("<i", out, off)[0]; off += 4
        kfs.append(np.frombuffer(out, np.int32, n, off).tolist()); off += 4 * n
    assert off == len(out)
    return ret, vec, (points, kfs)


# ---- search back-ends -----------------------------------------------------------------------------------------------------------------------
class OracleSearch:
    """The serial restatement of the reference (oracle/matcher_oracle.cpp): no GPU."""

    def __init__(self):
        from oracle import orb_oracle
        self.o = orb_oracle

    def projection(self, mode, v, q, qd, taken, assigned, ratio=0.0, check_ori=False, orb_dist=0, right=True):
        fo = self.o.FrameOracle(v["kps"], v["desc"], BOUNDS, v["right"] if right else None)
        n, a, _ = fo.search_by_projection(mode, q, qd, ratio, check_ori, taken, assigned, orb_dist)
        return n, a

    def window(self, v, q, qd, inv_s2, max_dist, right=True):
        fo = self.o.FrameOracle(v["kps"], v["desc"], BOUNDS, v["right"] if right else None)
        return fo.fuse_search(q, qd, inv_s2, max_dist)

    def triangulation(self, a, mpa, b, mpb, F, epi, stereo_only, check_ori):
        return self.o.search_for_triangulation(a["kps"], a["desc"], mpa, a["right"], a["fv"], b["kps"], b["desc"], mpb, b["right"], b["fv"], F, epi, SF,
                                               (SF * SF).astype(F32), stereo_only, check_ori)


class GpuSearch:
    """ydorbslam_amd.OrbMatcher: the direct C-ABI calls on the same flat problem."""

    def __init__(self):
        import ydorbslam_amd as y
        self.y = y

    def projection(self, mode, v, q, qd, taken, assigned, ratio=0.0, check_ori=False, orb_dist=0, right=True):
        fv = self.y.FrameView(v["kps"], v["desc"], BOUNDS, v["right"] if right else None)
        n, a, _ = self.y.OrbMatcher(ratio, check_ori).search_by_projection(mode, fv, q, qd, taken, assigned, orb_dist)
        return n, a

    def window(self, v, q, qd, inv_s2, max_dist, right=True):
        fv = self.y.FrameView(v["kps"], v["desc"], BOUNDS, v["right"] if right else None)
        return self.y.OrbMatcher().fuse_search(fv, q, qd, inv_s2, max_dist)

    def triangulation(self, a, mpa, b, mpb, F, epi, stereo_only, check_ori):
        FV = self.y.FeatureVector
        return self.y.OrbMatcher(0.6, check_ori).search_for_triangulation(a["kps"], a["desc"], mpa, a["right"], FV(*a["fv"]), b["kps"], b["desc"], mpb,
                                                                          b["right"], FV(*b["fv"]), F, epi, SF, (SF * SF).astype(F32), stereo_only)


# ---- shared pieces of the scenario builders ---------------------------------------------------------------------------------------------
def twin_xy(rng, u, v, r, sf_l, eps=(0.1, 0.6)):
    """Just outside the radius in x, well inside it in y; None when that leaves the image."""
    side = 1.0 if rng.random() < 0.5 else -1.0
    dx = float(r) + rng.uniform(*eps) * float(sf_l)
    for s in (side, -side):
        x = float(u) + s * dx
        if 2.0 < x < W - 2.0:
            return F32(x), F32(float(v) + rng.uniform(-0.3, 0.3))
    return None


def back_project(R, t, px, py, z):
    """World points whose camera coordinates R P + t project to (px, py) at depth z (float64 in, float32 out)."""
    Pc = np.stack([(px - float(CX)) / float(FX) * z, (py - float(CY)) / float(FY) * z, z], axis=1)
    return ((Pc - np.asarray(t, F64)) @ np.asarray(R, F64)).astype(F32)        # R^T (Pc - t), row-wise


def scatter(feats, rng, n, octaves=8):
    for _ in range(n):
        feats.add(rng.uniform(5, W - 5), rng.uniform(5, H - 5), rng.integers(0, octaves), rng.integers(0, 256, 32), angle=rng.uniform(0, 360))


def place_points(sc, rng, idx, kinds, R, t, O, level_frac=(0.1, 0.9), max_oct=7):
    """Positions, normals and distances of points idx so that the projection with (R, t), the distance to O and kinds[i] give the wanted
    predicate outcome.  Returns the level each point is meant to predict."""
    n = len(idx)
    px, py, z = rng.uniform(40, W - 40, n), rng.uniform(40, H - 40, n), rng.uniform(3.0, 8.0, n)
    for i, k in enumerate(kinds):
        if k == "behind":
            z[i] = -z[i]
        if k == "outside":
            px[i] = rng.choice([-60.0, W + 60.0]) if rng.random() < 0.5 else px[i]
            py[i] = rng.choice([-60.0, H + 60.0]) if 0 <= px[i] < W else py[i]
    P = back_project(R, t, px, py, z)
    PO = P.astype(F64) - np.asarray(O, F64)
    dist = np.linalg.norm(PO, axis=1)
    octv = rng.integers(0, max_oct + 1, n)
    octv[:min(n, 16)] = np.arange(min(n, 16)) % (max_oct + 1)       # every level occurs
    max_d = dist * 1.2 ** (octv - rng.uniform(*level_frac, n))
    min_d = max_d / float(SF[7])
    nrm = PO / dist[:, None]
    for i, k in enumerate(kinds):
        if k == "close":
            min_d[i] = dist[i] * 1.5
        if k == "far":
            max_d[i] = dist[i] / 1.5
        if k == "angle":
            nrm[i] = -nrm[i] if rng.random() < 0.5 else np.cross(nrm[i], [0.3, 0.5, 0.8]) / np.linalg.norm(np.cross(nrm[i], [0.3, 0.5, 0.8]))
        if k == "bad":
            sc.bad[idx[i]] = 1
    sc.pos[idx], sc.normal[idx], sc.min_d[idx], sc.max_d[idx] = P, nrm.astype(F32), min_d.astype(F32), max_d.astype(F32)
    return octv


def draw_kinds(rng, n, weights):
    names = list(weights)
    p = np.array([weights[k] for k in names], F64)
    kinds = [names[i] for i in rng.choice(len(names), n, p=p / p.sum())]
    for j, k in enumerate(names):                      # at least four of each
        for r in range(4):
            kinds[(j * 4 + r) % n] = k
    return kinds


# =================================================================================================================================
# The geometry shared by reloc, sim, fusesim and fuse: project with (R, t), measure the distance to a centre, predict the level, test
# the predicates.  centre / translation variants are the alternative readings the CPU tests discriminate.
# =================================================================================================================================
def geometry32(R, t, O, sc, idx, th, with_angle, with_ur=False):
    idx = np.asarray(idx, np.int64)
    P = sc.pos[idx]
    Pc = (gemv32(R, P) + np.asarray(t, F32)).astype(F32)
    u, v, z = pixel32(Pc)
    PO = (P - np.asarray(O, F32)).astype(F32)
    dist = norm32(PO)
    level = level32(sc.max_d[idx], dist)
    ok = (z >= F32(0)) & in_image(u, v) & (dist >= F32(0.8) * sc.min_d[idx]) & (dist <= F32(1.2) * sc.max_d[idx])
    if with_angle:
        nrm = sc.normal[idx].astype(F64)
        dot = PO[:, 0].astype(F64) * nrm[:, 0] + PO[:, 1].astype(F64) * nrm[:, 1] + PO[:, 2].astype(F64) * nrm[:, 2]
        ok &= dot >= 0.5 * dist.astype(F64)
    out = dict(u=u, v=v, z=z, level=level, r=(F32(th) * SF[level]).astype(F32), ok=ok, dist=dist)
    if with_ur:
        with np.errstate(all="ignore"):
            out["ur"] = (u - BF / z).astype(F32)
    return out


def geometry64(R, t, O, sc, idx, th, with_angle, with_ur=False, extra_R=0.0):
    """The same in plain float64, with the bound on |float - double| of u, v, ur, r that follows from the formats alone (docstring of
    test_statements_against_float64 in tests/test_matcher_adapters_cpu.py)."""
    idx = np.asarray(idx, np.int64)
    R, t, O = np.asarray(R, F64), np.asarray(t, F64), np.asarray(O, F64)
    P = sc.pos[idx].astype(F64)
    Pc = P @ R.T + t
    with np.errstate(all="ignore"):
        z = Pc[:, 2]
        u, v = float(FX) * Pc[:, 0] / z + float(CX), float(FY) * Pc[:, 1] / z + float(CY)
        PO = P - O
        dist = np.linalg.norm(PO, axis=1)
        max_d, min_d = sc.max_d[idx].astype(F64), sc.min_d[idx].astype(F64)
        lv = np.ceil(np.log(max_d / dist) / float(LOG_SF))
        level = np.where(~(lv >= 0), 0, np.where(lv >= 8, 7, lv)).astype(np.int32)
        ok = (z >= 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H) & (dist >= float(F32(0.8)) * min_d) & (dist <= float(F32(1.2)) * max_d)
        if with_angle:
            ok &= (PO * sc.normal[idx].astype(F64)).sum(axis=1) >= 0.5 * dist
        Pm = np.abs(P).max(axis=1)
        geo = 2 * EPS * ((2 + extra_R) * 1.7321 * Pm + np.abs(t).max()) / np.abs(z)
        tol = dict(u=float(FX) * geo * (1 + np.abs(u - float(CX)) / float(FX)) + 4 * EPS * (np.abs(u) + float(CX)),
                   v=float(FY) * geo * (1 + np.abs(v - float(CY)) / float(FY)) + 4 * EPS * (np.abs(v) + float(CY)))
        out = dict(u=u, v=v, z=z, level=level, r=float(th) * SF[level].astype(F64), ok=ok, dist=dist)
        tol["r"] = EPS * out["r"]
        if with_ur:
            out["ur"] = u - float(BF) / z
            tol["ur"] = tol["u"] + 4 * EPS * (np.abs(u) + float(BF) / np.abs(z))
    out["tol"] = tol
    return out


def sim_decompose32(S, t_over_scale=False):
    """SimProjection of orbMatcher.hpp (orbMatcher.cpp:241-247): scale = |first row of sR| (Mat::dot in double), R = sR / scale (a double
    division rounded to float), t = the last column AS IT IS - the header's reading, which this suite pins; ORB-SLAM2 divides t by the
    scale here (t_over_scale = True is that alternative) - and Ow = -R^T t."""
    S = np.asarray(S, F32)
    sR = S[:3, :3]
    scale = F32(np.sqrt((sR[0].astype(F64) * sR[0].astype(F64)).sum()))
    R = (sR.astype(F64) / F64(scale)).astype(F32)
    t = S[:3, 3].copy()
    if t_over_scale:
        t = (t.astype(F64) / F64(scale)).astype(F32)
    return R, t, gemv32(-(R.T), t)[0]


def sim_decompose64(S):
    S = np.asarray(S, F64)
    scale = np.linalg.norm(S[0, :3])
    R = S[:3, :3] / scale
    return R, S[:3, 3], -R.T @ S[:3, 3]


def fill_queries(g, select, flags, min_level=None, max_level=None, angle=None, ur=False, n=None):
    q = np.zeros(len(select) if n is None else n, QUERY_DTYPE)
    s = np.asarray(select, bool)
    q["u"][s], q["v"][s], q["r"][s], q["level"][s] = g["u"][s], g["v"][s], g["r"][s], g["level"][s]
    q["min_level"][s] = -1 if min_level is None else min_level[s]
    q["max_level"][s] = -1 if max_level is None else max_level[s]
    if angle is not None:
        q["angle"][s] = angle[s]
    if ur:
        q["ur"][s] = g["ur"][s]
    q["flags"][s] = np.asarray(flags)[s] if np.ndim(flags) else flags
    return q


# =================================================================================================================================
# mappoint: searchByProjectionInFrameAndMapPoint (orbMatcher.cpp:24-64)
# =================================================================================================================================
def scenario_mappoint(seed=101):
    rng = np.random.default_rng(seed)
    n_list, n_pool = 270, 24
    sc = Scene(n_list + n_pool, rng)
    store = Feats()
    thd = F32(1.0)
    f = Feats()
    lvl = rng.integers(0, 8, n_list)
    lvl[:24] = np.arange(24) % 8
    sc.track_level[:n_list] = lvl
    sc.in_view[:n_list] = rng.random(n_list) > 0.1
    sc.bad[:n_list] = rng.random(n_list) < 0.06
    cos = np.where(rng.random(n_list) < 0.5, rng.uniform(0.99, 0.9979, n_list), rng.uniform(0.9981, 1.0, n_list)).astype(F32)
    u, v, z = rng.uniform(40, W - 40, n_list).astype(F32), rng.uniform(40, H - 40, n_list).astype(F32), rng.uniform(3, 8, n_list).astype(F32)
    sc.track[:n_list] = np.stack([u, v, (u - BF / z).astype(F32), cos], axis=1)
    observed = rng.random(sc.n) < 0.65
    observed[n_list:] = np.arange(n_pool) % 2 == 0
    for p in np.flatnonzero(observed):
        sc.obs[p][0] = store.add(10, 10, 0, sc.desc[p], mp=p)
    pool = list(range(n_list, sc.n))
    for p in range(n_list):
        if rng.random() > 0.78:
            continue
        fac = F32(2.5) if cos[p] > 0.998 else F32(4.0)
        r = F32(F32(thd * fac) * SF[lvl[p]])
        at = twin_xy(rng, u[p], v[p], r, SF[lvl[p]])
        if at is None:
            continue
        c = rng.random()
        octave = lvl[p] if c < 0.75 else (max(lvl[p] - 1, 0) if c < 0.85 else min(lvl[p] + 1, 7))
        c = rng.random()
        right = -1.0 if c < 0.4 else (sc.track[p, 2] + rng.uniform(-0.5, 0.5) * r if c < 0.8 else sc.track[p, 2] + 3.0 * r)
        held = pool.pop() if (pool and rng.random() < 0.12) else -1
        f.add(at[0], at[1], octave, flip_bits(sc.desc[p], rng.integers(0, 40), rng), right=right, mp=held)
    scatter(f, rng, 60)
    sc.add_keyframe(np.eye(3), np.zeros(3), store)
    sc.frame = dict(T=np.eye(4, dtype=F32), **f.view())
    sc.args = dict(list=rng.permutation(n_list).astype(np.int32), thd=thd, ratio=F32(0.8))
    return sc


def statement_mappoint(sc, max_level_plus=0, swap_radii=False):
    """orbMatcher.cpp:24-64: a point takes part when it is in view and not bad; radius = thd * (2.5 when viewCos > 0.998, else 4.0)
    (getRadiusByViewCos :820-826), window radius * scaleFactor[level], levels level-1 .. level, ur with the same tolerance, flag bit 2 =
    the point has observations.  max_level_plus = 1 is the alternative reading level-1 .. level+1."""
    lst = sc.args["list"]
    live = (sc.in_view[lst] != 0) & (sc.bad[lst] == 0)
    lvl = sc.track_level[lst]
    big = sc.track[lst, 3].astype(F64) > 0.998
    if swap_radii:
        big = ~big
    radius = (sc.args["thd"] * np.where(big, F32(2.5), F32(4.0)).astype(F32)).astype(F32)
    g = dict(u=sc.track[lst, 0], v=sc.track[lst, 1], ur=sc.track[lst, 2], level=lvl, r=(radius * SF[lvl]).astype(F32))
    has_obs = np.array([len(sc.obs[p]) > 0 for p in lst])
    q = fill_queries(g, live, 1 | (has_obs.astype(np.int32) << 1), lvl - 1, lvl + max_level_plus, ur=True)
    q["rs"] = q["r"]
    qd = np.where(live[:, None], sc.desc[lst], 0).astype(np.uint8)
    fr = sc.frame
    taken = np.array([1 if (p >= 0 and len(sc.obs[p]) > 0) else 0 for p in fr["mp_of"]], np.uint8)
    return dict(q=q, qd=qd, taken=taken, live=live)


def double_mappoint(sc):
    lst = sc.args["list"]
    lvl = sc.track_level[lst]
    radius = float(sc.args["thd"]) * np.where(sc.track[lst, 3].astype(F64) > 0.998, 2.5, 4.0)
    r = radius * SF[lvl].astype(F64)
    z = np.zeros(len(lst))
    return dict(u=sc.track[lst, 0].astype(F64), v=sc.track[lst, 1].astype(F64), ur=sc.track[lst, 2].astype(F64), r=r, level=lvl,
                ok=(sc.in_view[lst] != 0) & (sc.bad[lst] == 0), tol=dict(u=z, v=z, ur=z, r=2 * EPS * r))


def expected_mappoint(sc, search):
    st = statement_mappoint(sc)
    fr, lst = sc.frame, sc.args["list"]
    n, assigned = search.projection(0, fr, st["q"], st["qd"], st["taken"], np.full(len(fr["kps"]), -1, np.int32), ratio=float(sc.args["ratio"]))
    want = fr["mp_of"].copy()
    hit = assigned >= 0
    want[hit] = lst[assigned[hit]]
    q = st["q"]
    live = st["live"]
    held = fr["mp_of"] >= 0
    counts = dict(matches=int(hit.sum()), not_in_view=int((sc.in_view[lst] == 0).sum()), bad=int((sc.bad[lst] != 0).sum()),
                  level0=int((live & (q["level"] == 0)).sum()), level7=int((live & (q["level"] == 7)).sum()),
                  level0_matched=int((q["level"][assigned[hit]] == 0).sum()), level7_matched=int((q["level"][assigned[hit]] == 7).sum()),
                  stereo_matched=int((hit & (fr["right"] > 0)).sum()), observed=int((q["flags"] == 3).sum()), unobserved=int((q["flags"] == 1).sum()),
                  radius_2_5=int((live & (q["r"] == (F32(sc.args["thd"] * F32(2.5)) * SF[q["level"]]).astype(F32))).sum()),
                  radius_4_0=int((live & (q["r"] == (F32(sc.args["thd"] * F32(4.0)) * SF[q["level"]]).astype(F32))).sum()),
                  prefilled_taken=int((held & (st["taken"] == 1)).sum()), prefilled_free=int((held & (st["taken"] == 0)).sum()),
                  prefilled_free_overwritten=int((held & (st["taken"] == 0) & hit).sum()))
    return n, want, State(sc), counts


def blob_mappoint(sc):
    return sc.world_blob() + point_list_blob(sc.args["list"]) + struct.pack("<2f", sc.args["thd"], sc.args["ratio"])


# =================================================================================================================================
# reloc: searchByProjectionInKeyFrameAndCurrentFrame (orbMatcher.cpp:156-239)
# =================================================================================================================================
def scenario_reloc(seed=202, orb_dist=100, check_ori=True):
    rng = np.random.default_rng(seed)
    nq, n_pool = 280, 16
    sc = Scene(nq + n_pool, rng)
    R = (rot([0, 1, 0], 20.0) @ rot([1, 0, 0], 5.0)).astype(F32)
    t = np.array([1.0, 0.2, -0.3], F32)
    T = np.eye(4, dtype=F32)
    T[:3, :3], T[:3, 3] = R, t
    Ow = gemv32(-R, t)[0]                                           # the centre as the reference writes it at :160
    thd = F32(10.0)
    kinds = draw_kinds(rng, nq, dict(ok=0.66, behind=0.06, outside=0.06, close=0.05, far=0.05, null=0.04, bad=0.04, found=0.04))
    idx = np.arange(nq)
    place_points(sc, rng, idx, kinds, R, t, Ow, max_oct=6)
    kf, cur, store = Feats(), Feats(), Feats()
    for p in range(nq):
        kf.add(rng.uniform(5, W - 5), rng.uniform(5, H - 5), rng.integers(0, 8), rng.integers(0, 256, 32), angle=rng.uniform(0, 360),
               mp=-1 if kinds[p] == "null" else p)
    g = geometry32(R, t, Ow, sc, idx, thd, False)
    pool = list(range(nq, sc.n))
    odd = 0
    for p in range(nq):
        if kinds[p] == "null" or rng.random() > 0.85:
            continue
        lv = int(g["level"][p])
        at = twin_xy(rng, g["u"][p], g["v"][p], g["r"][p], SF[lv]) if np.isfinite(g["u"][p]) and in_image(g["u"][p], g["v"][p]) else None
        if at is None:
            continue
        octave = min(lv + 1, 7) if rng.random() < 0.85 else lv
        bits = rng.integers(0, 36) if rng.random() < 0.6 else rng.integers(45, 90)
        a = kf.rows[p][3]
        if kinds[p] == "ok" and bits < 36 and octave == lv + 1 and odd < 9:     # a few matches off the main rotation bin: culled with checkOri
            a = F32((float(a) - (90.0, 180.0, 270.0)[odd % 3]) % 360.0)
            odd += 1
        held = pool.pop() if (pool and kinds[p] == "ok" and rng.random() < 0.08) else -1
        cur.add(at[0], at[1], octave, flip_bits(sc.desc[p], bits, rng), angle=a, mp=held)
    scatter(cur, rng, 60)
    for p in range(nq, sc.n):
        if p % 2:
            sc.obs[p][1] = store.add(10, 10, 0, sc.desc[p], mp=p)
    sc.add_keyframe(np.eye(3), np.zeros(3), kf)
    sc.add_keyframe(np.eye(3), np.zeros(3), store)
    sc.link()
    sc.frame = dict(T=T, **cur.view())
    sc.args = dict(kf=0, found=np.array([p for p in range(nq) if kinds[p] == "found"], np.int32), thd=thd, orb_dist=orb_dist, check_ori=check_ori, kinds=kinds)
    return sc


def statement_reloc(sc, centre="R"):
    """orbMatcher.cpp:156-239: the frame's rotation and translation project every matched point of the keyframe that is set, not bad and
    not in `found`; the camera centre is -R t AS WRITTEN at :160 (SURVEY.md:291; centre = "Rt" is the alternative -R^T t); a point takes
    part when z >= 0, the pixel is inside the image and the distance to that centre is inside the invariance; window thd *
    scaleFactor[predicted level], levels predicted-1 .. predicted+1, the keyframe keypoint's angle, flags 3."""
    T = sc.frame["T"]
    R, t = T[:3, :3], T[:3, 3]
    Ow = gemv32(-R if centre == "R" else -(R.T), t)[0]
    kf = sc.kfs[sc.args["kf"]]
    mp = kf["mp_of"]
    found = set(sc.args["found"].tolist())
    live = np.array([p >= 0 and not sc.bad[p] and p not in found for p in mp])
    g = geometry32(R, t, Ow, sc, np.maximum(mp, 0), sc.args["thd"], False)
    sel = live & g["ok"]
    q = fill_queries(g, sel, 3, g["level"] - 1, g["level"] + 1, angle=kf["kps"]["angle"])
    qd = np.where(sel[:, None], sc.desc[np.maximum(mp, 0)], 0).astype(np.uint8)
    return dict(q=q, qd=qd, taken=(sc.frame["mp_of"] >= 0).astype(np.uint8), live=live, g=g)


def double_reloc(sc):
    T = sc.frame["T"].astype(F64)
    mp = sc.kfs[sc.args["kf"]]["mp_of"]
    return geometry64(T[:3, :3], T[:3, 3], -T[:3, :3] @ T[:3, 3], sc, np.maximum(mp, 0), sc.args["thd"], False)


def expected_reloc(sc, search):
    st = statement_reloc(sc)
    fr, kf = sc.frame, sc.kfs[sc.args["kf"]]
    n, assigned = search.projection(2, fr, st["q"], st["qd"], st["taken"], np.full(len(fr["kps"]), -2, np.int32), check_ori=sc.args["check_ori"],
                                    orb_dist=sc.args["orb_dist"])
    want = fr["mp_of"].copy()
    want[assigned >= 0] = kf["mp_of"][assigned[assigned >= 0]]
    want[assigned == -1] = -1
    g, live, kinds = st["g"], st["live"], np.array(sc.args["kinds"])
    with np.errstate(all="ignore"):
        counts = dict(matches=int((assigned >= 0).sum()), culled=int((assigned == -1).sum()), found_skipped=len(sc.args["found"]),
                      null=int((kf["mp_of"] < 0).sum()), bad=int(sc.bad[np.maximum(kf["mp_of"], 0)][kf["mp_of"] >= 0].sum()),
                      behind=int((live & ~(g["z"] >= 0)).sum()), outside=int((live & (g["z"] >= 0) & ~in_image(g["u"], g["v"])).sum()),
                      too_close=int((live & (kinds == "close") & ~g["ok"]).sum()), too_far=int((live & (kinds == "far") & ~g["ok"]).sum()),
                      taken_any=int(st["taken"].sum()), taken_unobserved=int(sum(1 for p in fr["mp_of"] if p >= 0 and not sc.obs[p])))
    return n, want, State(sc), counts


def blob_reloc(sc):
    a = sc.args
    return sc.world_blob() + struct.pack("<i", a["kf"]) + point_list_blob(a["found"]) + struct.pack("<fii", a["thd"], a["orb_dist"], int(a["check_ori"]))


# =================================================================================================================================
# sim / fusesim: searchByProjectionInSim (orbMatcher.cpp:240-302) and fuseBySim3 (:746-807) share the Sim3 decomposition and the query
# =================================================================================================================================
def _sim_pose(scale):
    R = rot([0.2, 1.0, 0.1], 15.0)
    t = np.array([1.5, -0.6, 0.9], F64)            # long enough for t / scale to move the centre by decimetres at scales 0.8 and 1.3
    S = np.eye(4, dtype=F32)
    S[:3, :3], S[:3, 3] = (scale * R).astype(F32), t.astype(F32)
    return S


def scenario_sim(scale=1.0, seed=303):
    rng = np.random.default_rng(seed + int(round(scale * 10)))
    n_list, n_pool = 260, 20
    sc = Scene(n_list + n_pool, rng)
    S = _sim_pose(scale)
    R, t, Ow = sim_decompose32(S)
    th = 10
    kinds = draw_kinds(rng, n_list, dict(ok=0.62, behind=0.05, outside=0.05, close=0.04, far=0.04, angle=0.06, null=0.04, bad=0.04, found=0.06))
    idx = np.arange(n_list)
    place_points(sc, rng, idx, kinds, R, t, Ow)
    g = geometry32(R, t, Ow, sc, idx, th, True)
    kf = Feats()
    matched = []
    pool = list(range(n_list, sc.n))
    for p in range(n_list):
        if kinds[p] == "null" or (kinds[p] != "found" and rng.random() > 0.85) or not (np.isfinite(g["u"][p]) and in_image(g["u"][p], g["v"][p])):
            continue                                   # (a found point has a free twin too: only the found-set keeps it from being matched again)
        lv = int(g["level"][p])
        at = twin_xy(rng, g["u"][p], g["v"][p], g["r"][p], SF[lv])
        if at is None:
            continue
        c = rng.random()
        octave = lv if c < 0.7 else (max(lv - 1, 0) if c < 0.9 else min(lv + 1, 7))
        bits = rng.integers(0, 46) if rng.random() < 0.8 else rng.integers(55, 80)
        if kinds[p] == "found":
            octave, bits = lv, rng.integers(0, 30)
        kf.add(at[0], at[1], octave, flip_bits(sc.desc[p], bits, rng))
        matched.append(pool.pop() if (pool and kinds[p] == "ok" and rng.random() < 0.08) else -1)      # a taken slot
    for p in range(n_list):
        if kinds[p] == "found":                                                                         # the caller already holds these
            kf.add(rng.uniform(5, W - 5), rng.uniform(5, H - 5), rng.integers(0, 8), rng.integers(0, 256, 32))
            matched.append(p)
    scatter(kf, rng, 50)
    matched += [-1] * (len(kf) - len(matched))
    sc.add_keyframe(R, t, kf)
    lst = np.array([-1 if kinds[p] == "null" else p for p in range(n_list)], np.int32)[rng.permutation(n_list)]
    sc.args = dict(kf=0, S=S, list=lst, matched=np.array(matched, np.int32), th=th, scale=scale, kinds=kinds)
    return sc


def statement_sim(sc, t_over_scale=False, flags_ok=3, ignore_found=False):
    """orbMatcher.cpp:240-302 / :746-807 over SimProjection: a list entry takes part when it is set, not bad and not in the found set; it
    is projected with R and t of the decomposition, its distance is measured to Ow = -R^T t, the level predicted from it, and it is
    searched when z >= 0, the pixel is inside the image, the distance is inside the invariance and PO . normal >= 0.5 dist (Mat::dot and
    the right side in double); window th * scaleFactor[level], explicit level window predicted-1 .. predicted on the device."""
    R, t, Ow = sim_decompose32(sc.args["S"], t_over_scale)
    lst = sc.args["list"]
    found = sc.args["found_set"] if "found_set" in sc.args else set(int(p) for p in sc.args["matched"] if p >= 0)
    if ignore_found:                                   # not a reading of the reference: used to show that the found set matters to a scenario
        found = set()
    live = np.array([p >= 0 and not sc.bad[p] and p not in found for p in lst])
    g = geometry32(R, t, Ow, sc, np.maximum(lst, 0), F32(sc.args["th"]), True)
    sel = live & g["ok"]
    q = fill_queries(g, live, np.where(sel, flags_ok, 0))       # the query is filled for every live entry; only the flags say whether it is searched
    qd = np.where(live[:, None], sc.desc[np.maximum(lst, 0)], 0).astype(np.uint8)
    return dict(q=q, qd=qd, live=live, sel=sel, g=g)


def double_sim(sc):
    R, t, Ow = sim_decompose64(sc.args["S"])
    return geometry64(R, t, Ow, sc, np.maximum(sc.args["list"], 0), sc.args["th"], True, extra_R=2.0)


def _predicate_counts(sc, live, g, kinds_of_list):
    k = np.array(kinds_of_list)
    with np.errstate(all="ignore"):
        return dict(behind=int((live & ~(g["z"] >= 0)).sum()), outside=int((live & (g["z"] >= 0) & ~in_image(g["u"], g["v"])).sum()),
                    too_close=int((live & (k == "close") & ~g["ok"]).sum()), too_far=int((live & (k == "far") & ~g["ok"]).sum()),
                    angle=int((live & (k == "angle") & ~g["ok"]).sum()))


def expected_sim(sc, search):
    st = statement_sim(sc)
    kf, lst, matched = sc.kfs[sc.args["kf"]], sc.args["list"], sc.args["matched"]
    taken = (matched >= 0).astype(np.uint8)
    n, assigned = search.projection(7, kf, st["q"], st["qd"], taken, np.full(len(matched), -1, np.int32))
    want = matched.copy()
    want[assigned >= 0] = lst[assigned[assigned >= 0]]
    g, live = st["g"], st["live"]
    alt = statement_sim(sc, ignore_found=True)         # without the found set, its members would be matched a second time
    _, again = search.projection(7, kf, alt["q"], alt["qd"], taken, np.full(len(matched), -1, np.int32))
    in_found = set(int(p) for p in matched if p >= 0)
    with np.errstate(all="ignore"):
        counts = dict(matches=int((assigned >= 0).sum()), prefilled=int(taken.sum()),
                      found_would_match=int(sum(1 for a in again if a >= 0 and int(lst[a]) in in_found)), found_skipped=int(sum(1 for p in lst if p >= 0 and p in set(matched.tolist()))),
                      null=int((lst < 0).sum()), bad=int(sum(1 for p in lst if p >= 0 and sc.bad[p])),
                      behind=int((live & ~(g["z"] >= 0)).sum()), outside=int((live & (g["z"] >= 0) & ~in_image(g["u"], g["v"])).sum()),
                      invariance=int((live & (g["z"] >= 0) & in_image(g["u"], g["v"]) &
                                      ~((g["dist"] >= F32(0.8) * sc.min_d[np.maximum(lst, 0)]) & (g["dist"] <= F32(1.2) * sc.max_d[np.maximum(lst, 0)]))).sum()),
                      angle=int((live & ~g["ok"] & np.array([p >= 0 and sc.args["kinds"][p] == "angle" for p in lst])).sum()),
                      rejected=int((live & ~st["sel"]).sum()))
    return n, want, State(sc), counts


def blob_sim(sc):
    a = sc.args
    return sc.world_blob() + struct.pack("<i", a["kf"]) + a["S"].tobytes() + point_list_blob(a["list"]) + point_list_blob(a["matched"]) + struct.pack("<i", a["th"])


def _fuse_scene(rng, sc, n_list, kinds, g, th, stereo, by_obs, chi_eps):
    """The target keyframe (index 0) and two storage keyframes (1, 2) of a fuse scenario.  Fates of a searched point by what its best
    feature holds: nothing (added), a point with more / fewer / as many observations (by_obs: the one with fewer is replaced, ties
    replace the held one; otherwise the listed point is always the one replaced), a bad point (counted only).  `share`: the point is in
    the keyframe already.  Returns the list order with duplicates of added and of replaced points appended."""
    kf, s1, s2 = Feats(), Feats(), Feats()
    held_next = n_list
    dup = []
    fates = {}
    for p in range(n_list):
        k = kinds[p]
        if k == "null":
            continue
        n_own = 2 if (by_obs and rng.random() < 0.5) else 1
        s1.add(10, 10, 0, sc.desc[p], mp=p)
        if n_own == 2:
            s2.add(10, 10, 0, sc.desc[p], mp=p)
        if k == "found":                                      # held by a keyframe feature far from its projection
            kf.add(rng.uniform(5, W - 5), rng.uniform(5, H - 5), rng.integers(0, 8), rng.integers(0, 256, 32), mp=p)
            continue
        if rng.random() > 0.85 or not (np.isfinite(g["u"][p]) and in_image(g["u"][p], g["v"][p])):
            continue
        lv = int(g["level"][p])
        at = twin_xy(rng, g["u"][p], g["v"][p], g["r"][p], SF[lv], chi_eps)
        if at is None:
            continue
        c = rng.random()
        octave = lv if c < 0.85 else max(lv - 1, 0)
        bits = rng.integers(0, 46) if rng.random() < 0.85 else rng.integers(55, 80)
        right = -1.0
        if stereo and rng.random() < 0.5 and g["z"][p] > 0:
            right = float(g["u"][p]) - float(BF) / float(g["z"][p]) + rng.uniform(-0.2, 0.2)      # the projected right x, nearly
        fate = rng.choice(["empty", "more", "fewer", "equal", "badheld"], p=[0.3, 0.25, 0.2, 0.1, 0.15]) if k == "ok" else "empty"
        held = -1
        if fate != "empty" and held_next < sc.n:
            held = held_next
            held_next += 1
            sc.pos[held], sc.normal[held], sc.min_d[held], sc.max_d[held] = sc.pos[p], sc.normal[p], sc.min_d[p], sc.max_d[p]
            extra = {"more": n_own, "fewer": n_own - 2, "equal": n_own - 1, "badheld": 1}[fate]      # observations beside the target keyframe
            if extra >= 1:
                s1.add(10, 10, 0, sc.desc[held], mp=held)
            if extra >= 2:
                s2.add(10, 10, 0, sc.desc[held], mp=held)
            if fate == "badheld":
                sc.bad[held] = 1
        elif fate != "empty":
            fate = "empty"
        kf.add(at[0], at[1], octave, flip_bits(sc.desc[p], bits, rng), right=right, mp=held)
        if k == "ok" and bits < 46 and octave == lv:
            fates[p] = fate
            if fate in ("empty", "more") and rng.random() < 0.4:
                dup.append(p)
    scatter(kf, rng, 40)
    sc.add_keyframe(*sc.args["pose"], kf)
    sc.add_keyframe(np.eye(3), np.zeros(3), s1)
    sc.add_keyframe(np.eye(3), np.zeros(3), s2)
    sc.link()
    lst = [-1 if kinds[p] == "null" else p for p in rng.permutation(n_list)]
    sc.args["planned"] = fates
    return np.array(lst + dup, np.int32)


def scenario_fusesim(scale=1.0, seed=404):
    rng = np.random.default_rng(seed + int(round(scale * 10)))
    n_list = 200
    sc = Scene(290, rng)
    S = _sim_pose(scale)
    R, t, Ow = sim_decompose32(S)
    th = F32(4.0)
    kinds = draw_kinds(rng, n_list, dict(ok=0.62, behind=0.05, outside=0.05, close=0.04, far=0.04, angle=0.06, null=0.04, bad=0.04, found=0.06))
    place_points(sc, rng, np.arange(n_list), kinds, R, t, Ow)
    g = geometry32(R, t, Ow, sc, np.arange(n_list), th, True)
    sc.args = dict(kf=0, S=S, th=th, scale=scale, pose=(R, t))
    sc.args["list"] = _fuse_scene(rng, sc, n_list, kinds, g, th, True, False, (0.1, 0.6))
    sc.args["found_set"] = set(int(p) for p in sc.kfs[0]["mp_of"] if p >= 0)
    sc.args["kinds"] = kinds
    return sc


def expected_fusesim(sc, search):
    """fuseBySim3: the found set is the keyframe's matched points BEFORE the loop; right_x is nulled and the inverse-sigma table is zero,
    so every feature takes the monocular branch of a test that always passes; then, in list order: not found or bad at its turn ->
    nothing; the feature holds a point -> the listed point is replaced by it unless that one is bad; empty -> observation added on both
    sides; every searched entry with a best feature counts."""
    st = statement_sim(sc, flags_ok=1)
    kf_i, lst = sc.args["kf"], sc.args["list"]
    _, best = search.window(sc.kfs[kf_i], st["q"], st["qd"], np.zeros(8, F32), 50, right=False)
    S_ = State(sc)
    n = 0
    counts = dict(added=0, replaced=0, bad_held=0, self_again=0, bad_at_turn=0, found_skipped=int(sum(1 for p in lst if p >= 0 and p in sc.args["found_set"])),
                  stereo_feature=0, rejected=int((st["live"] & ~st["sel"]).sum()), null=int((lst < 0).sum()))
    for i, p in enumerate(lst):
        if best[i] < 0 or not (st["q"]["flags"][i] & 1):
            continue
        if S_.bad[p]:
            counts["bad_at_turn"] += 1
            continue
        held = S_.kf_mps[kf_i][best[i]]
        counts["stereo_feature"] += int(sc.kfs[kf_i]["right"][best[i]] >= 0)
        if held >= 0:
            if not S_.bad[held]:
                counts["self_again" if held == p else "replaced"] += 1
                S_.replace(p, held)
            else:
                counts["bad_held"] += 1
        else:
            S_.add(p, kf_i, int(best[i]))
            counts["added"] += 1
        n += 1
    counts["matches"] = n
    return n, np.zeros(0, np.int32), S_, counts


def blob_fusesim(sc):
    a = sc.args
    return sc.world_blob() + struct.pack("<i", a["kf"]) + a["S"].tobytes() + point_list_blob(a["list"]) + struct.pack("<f", a["th"])


# =================================================================================================================================
# fuse: fuseByProjection, flat form (orbMatcher.cpp:682-745)
# =================================================================================================================================
def scenario_fuse(seed=505):
    rng = np.random.default_rng(seed)
    n_list = 200
    sc = Scene(295, rng)
    R, t = rot([0.1, 1.0, 0.3], 12.0).astype(F32), np.array([0.3, 0.1, -0.2], F32)
    Ow = gemv32(-(R.T), t)[0]
    th = F32(2.0)                                             # (th + 0.35)^2 < 5.99: a twin one level down fails the chi-square test
    kinds = draw_kinds(rng, n_list, dict(ok=0.64, behind=0.05, outside=0.05, close=0.04, far=0.04, angle=0.06, null=0.03, bad=0.04, found=0.05))
    place_points(sc, rng, np.arange(n_list), kinds, R, t, Ow)
    g = geometry32(R, t, Ow, sc, np.arange(n_list), th, True, True)
    sc.args = dict(kf=0, th=th, pose=(R, t))
    sc.args["list"] = _fuse_scene(rng, sc, n_list, kinds, g, th, True, True, (0.1, 0.35))
    sc.args["kinds"] = kinds
    return sc


def statement_fuse(sc):
    """orbMatcher.cpp:682-745, pass 1: an entry takes part when it is set, not bad and not in the keyframe; projection with the keyframe's
    rotation and translation, ur = u - bf / z, distance to the keyframe's stored centre, predicted level, window th * scaleFactor[level];
    flags 1 when z >= 0, inside the image, inside the distance invariance and PO . normal >= 0.5 dist."""
    kf_i = sc.args["kf"]
    kf, lst = sc.kfs[kf_i], sc.args["list"]
    live = np.array([p >= 0 and not sc.bad[p] and kf_i not in sc.obs[p] for p in lst])
    g = geometry32(kf["R"], kf["t"], kf["O"], sc, np.maximum(lst, 0), sc.args["th"], True, True)
    sel = live & g["ok"]
    q = fill_queries(g, live, np.where(sel, 1, 0), ur=True)
    qd = np.where(live[:, None], sc.desc[np.maximum(lst, 0)], 0).astype(np.uint8)
    return dict(q=q, qd=qd, live=live, sel=sel, g=g)


def double_fuse(sc):
    kf = sc.kfs[sc.args["kf"]]
    R, t = kf["R"].astype(F64), kf["t"].astype(F64)
    return geometry64(R, t, kf["O"], sc, np.maximum(sc.args["list"], 0), sc.args["th"], True, True)


def expected_fuse(sc, search):
    """Pass 3 in list order: bad or in the keyframe at its turn -> skipped; the best feature holds a point that is not bad -> the one with
    fewer observations is replaced, ties replace the held one (<=); holds a bad point -> counted only; empty -> added on both sides."""
    st = statement_fuse(sc)
    kf_i, lst = sc.args["kf"], sc.args["list"]
    kf = sc.kfs[kf_i]
    _, best = search.window(kf, st["q"], st["qd"], INV_S2, 50)
    S_ = State(sc)
    n = 0
    in_kf_before = int(sum(1 for p in lst if p >= 0 and not sc.bad[p] and kf_i in sc.obs[p]))
    counts = dict(added=0, held_more=0, held_fewer=0, held_equal=0, bad_held=0, bad_at_turn=0, in_kf_at_turn=0, in_kf_before=in_kf_before,
                  stereo_feature=0, mono_feature=0, null=int((lst < 0).sum()))
    counts.update(_predicate_counts(sc, st["live"], st["g"], [sc.args["kinds"][p] if p >= 0 else "null" for p in lst]))
    for i, p in enumerate(lst):
        if best[i] < 0 or not (st["q"]["flags"][i] & 1):
            continue
        if S_.bad[p]:
            counts["bad_at_turn"] += 1
            continue
        if kf_i in S_.obs[p]:
            counts["in_kf_at_turn"] += 1
            continue
        held = S_.kf_mps[kf_i][best[i]]
        counts["stereo_feature" if kf["right"][best[i]] >= 0 else "mono_feature"] += 1
        if held >= 0:
            if S_.bad[held]:
                counts["bad_held"] += 1
            elif S_.n_obs(held) > S_.n_obs(p):
                counts["held_more"] += 1
                S_.replace(p, held)
            else:
                counts["held_equal" if S_.n_obs(held) == S_.n_obs(p) else "held_fewer"] += 1
                S_.replace(held, p)
        else:
            S_.add(p, kf_i, int(best[i]))
            counts["added"] += 1
        n += 1
    counts["matches"] = n
    return n, np.zeros(0, np.int32), S_, counts


def blob_fuse(sc):
    a = sc.args
    return sc.world_blob() + struct.pack("<i", a["kf"]) + point_list_blob(a["list"]) + struct.pack("<f", a["th"])


# =================================================================================================================================
# sim3: searchBySim3 (orbMatcher.cpp:566-681)
# =================================================================================================================================
def scenario_sim3(seed=606):
    rng = np.random.default_rng(seed)
    n_pairs = 140
    sc = Scene(2 * n_pairs + 10, rng)
    R1, t1 = np.eye(3, dtype=F32), np.zeros(3, F32)
    R2, t2 = rot([0.1, 1.0, 0.0], 5.0).astype(F32), np.array([-0.3, 0.05, 0.1], F32)
    th = F32(10.0)
    kinds = draw_kinds(rng, n_pairs, dict(agree=0.46, nodesc=0.1, done1=0.08, done1_absent=0.06, done2=0.08, behind=0.05, outside=0.05, close=0.04,
                                          far=0.04, bad=0.04))
    A, B = np.arange(n_pairs), np.arange(n_pairs) + n_pairs
    geo = ["ok" if k not in ("behind", "outside", "close", "far", "bad") else k for k in kinds]
    place_points(sc, rng, A, geo, R2, t2, -(R2.astype(F64).T @ t2.astype(F64)), level_frac=(0.3, 0.7))       # A is judged in keyframe 2 by |Pc|
    sc.pos[B], sc.desc[B] = sc.pos[A], sc.desc[A]
    sc.bad[B] = 0
    f1, f2 = Feats(), Feats()
    matched = {}
    # B is judged in keyframe 1 (identity pose): distance = |P|
    d1 = np.linalg.norm(sc.pos[B].astype(F64), axis=1)
    oct_b = rng.integers(0, 8, n_pairs)
    sc.max_d[B] = (d1 * 1.2 ** (oct_b - rng.uniform(0.3, 0.7, n_pairs))).astype(F32)
    sc.min_d[B] = sc.max_d[B] / SF[7]
    gA = _sim3_direction32(sc, A, R2, t2, th)
    gB = _sim3_direction32(sc, B, R1, t1, th)
    pending = []
    for k in range(n_pairs):
        i = j = None
        if np.isfinite(gB["u"][k]) and in_image(gB["u"][k], gB["v"][k]):
            at = twin_xy(rng, gB["u"][k], gB["v"][k], gB["r"][k], SF[gB["level"][k]])
            if at is not None:
                i = f1.add(at[0], at[1], max(int(gB["level"][k]) - int(rng.random() < 0.3), 0), flip_bits(sc.desc[B[k]], rng.integers(0, 60), rng), mp=A[k])
        if i is None:
            i = f1.add(rng.uniform(5, W - 5), rng.uniform(5, H - 5), rng.integers(0, 8), rng.integers(0, 256, 32), mp=A[k])
        if np.isfinite(gA["u"][k]) and in_image(gA["u"][k], gA["v"][k]):
            at = twin_xy(rng, gA["u"][k], gA["v"][k], gA["r"][k], SF[gA["level"][k]])
            if at is not None:
                j = f2.add(at[0], at[1], max(int(gA["level"][k]) - int(rng.random() < 0.3), 0), flip_bits(sc.desc[A[k]], rng.integers(0, 60), rng), mp=B[k])
        if j is None:
            j = f2.add(rng.uniform(5, W - 5), rng.uniform(5, H - 5), rng.integers(0, 8), rng.integers(0, 256, 32), mp=B[k])
        if kinds[k] == "nodesc":                     # B's own descriptor is unrelated: the way back finds nothing
            sc.desc[B[k]] = rng.integers(0, 256, 32)
        if kinds[k] == "done1":
            matched[i] = B[k]
        if kinds[k] == "done1_absent":
            matched[i] = 2 * n_pairs + len([m for m in matched.values() if m >= 2 * n_pairs]) % 10
        if kinds[k] == "done2":
            pending.append(B[k])
    for p in pending:                                # held by the caller at a first-keyframe feature without a pair: marks done2 only
        i = f1.add(rng.uniform(5, W - 5), rng.uniform(5, H - 5), rng.integers(0, 8), rng.integers(0, 256, 32))
        matched[i] = p
    scatter(f1, rng, 30)
    scatter(f2, rng, 30)
    sc.add_keyframe(R1, t1, f1)
    sc.add_keyframe(R2, t2, f2)
    sc.link()
    m12 = np.full(len(f1), -1, np.int32)
    for i, p in matched.items():
        m12[i] = p
    sc.args = dict(kf1=0, kf2=1, matched=m12, th=th, kinds=kinds)
    return sc


def _sim3_direction32(sc, idx, R, t, th):
    P = sc.pos[idx]
    Pc = (gemv32(R, P) + np.asarray(t, F32)).astype(F32)
    u, v, z = pixel32(Pc)
    dist = norm32(Pc)
    level = level32(sc.max_d[idx], dist)
    ok = (z >= F32(0)) & in_image(u, v) & (dist >= F32(0.8) * sc.min_d[idx]) & (dist <= F32(1.2) * sc.max_d[idx])
    return dict(u=u, v=v, z=z, level=level, r=(F32(th) * SF[level]).astype(F32), ok=ok, dist=dist)


def statement_sim3(sc):
    """orbMatcher.cpp:566-681 as written: done1[i] where the caller's vector is set, done2[idx] for that point's index in the second
    keyframe when it has one; each direction projects the other keyframe's points that are set, not done and not bad with the TARGET
    keyframe's own pose, distance = |Pc| (cv::norm in double), predicted level, window th * scaleFactor[level], flags 1 when z >= 0,
    inside the image and inside the distance invariance (no viewing angle)."""
    k1, k2 = sc.kfs[sc.args["kf1"]], sc.kfs[sc.args["kf2"]]
    m12 = sc.args["matched"]
    done1, done2 = np.zeros(len(k1["kps"]), bool), np.zeros(len(k2["kps"]), bool)
    for i, p in enumerate(m12):
        if p >= 0:
            done1[i] = True
            j = sc.obs[p].get(sc.args["kf2"], -1)
            if j >= 0:
                done2[j] = True
    out = []
    for src, done, dst in ((k1, done1, k2), (k2, done2, k1)):
        mp = src["mp_of"]
        live = (mp >= 0) & ~done & (sc.bad[np.maximum(mp, 0)] == 0)
        g = _sim3_direction32(sc, np.maximum(mp, 0), dst["R"], dst["t"], sc.args["th"])
        q = fill_queries(g, live, np.where(live & g["ok"], 1, 0))
        out.append(dict(q=q, qd=np.where(live[:, None], sc.desc[np.maximum(mp, 0)], 0).astype(np.uint8), live=live, g=g))
    return out, done1, done2


def double_sim3(sc):
    res = []
    for src, dst in ((sc.args["kf1"], sc.args["kf2"]), (sc.args["kf2"], sc.args["kf1"])):
        mp = np.maximum(sc.kfs[src]["mp_of"], 0)
        R, t = sc.kfs[dst]["R"].astype(F64), sc.kfs[dst]["t"].astype(F64)
        res.append(geometry64(R, t, -R.T @ t, sc, mp, sc.args["th"], False))     # |P - (-R^T t)| = |R P + t|
    return res


def expected_sim3(sc, search):
    (d12, d21), done1, done2 = statement_sim3(sc)
    k1, k2 = sc.kfs[sc.args["kf1"]], sc.kfs[sc.args["kf2"]]
    zero = np.zeros(8, F32)
    _, b12 = search.window(k2, d12["q"], d12["qd"], zero, 100, right=False)
    _, b21 = search.window(k1, d21["q"], d21["qd"], zero, 100, right=False)
    want = sc.args["matched"].copy()
    n = one_way = 0
    for i in range(len(k1["kps"])):
        j = b12[i]
        if j >= 0 and b21[j] == i:
            want[i] = k2["mp_of"][j]
            n += 1
        elif j >= 0:
            one_way += 1
    absent = int(sum(1 for p in sc.args["matched"] if p >= 0 and sc.args["kf2"] not in sc.obs[p]))
    counts = dict(matches=n, one_way=one_way, done1=int(done1.sum()), done2=int(done2.sum()), absent_from_kf2=absent,
                  one_way_because_done2=int(sum(1 for i in range(len(k1["kps"])) if b12[i] >= 0 and done2[b12[i]])),
                  rejected12=int((d12["live"] & ~d12["g"]["ok"]).sum()), rejected21=int((d21["live"] & ~d21["g"]["ok"]).sum()))
    return n, want, State(sc), counts


def blob_sim3(sc):
    a = sc.args
    return sc.world_blob() + struct.pack("<2i", a["kf1"], a["kf2"]) + point_list_blob(a["matched"]) + struct.pack("<f", a["th"])


# =================================================================================================================================
# tri: searchForTriangulation, flat form (orbMatcher.cpp:463-565)
# =================================================================================================================================
def scenario_tri(seed=707, stereo_only=False, check_ori=True):
    """Keyframe 2 sees keyframe 1's features moved by (11, -3) px, so F12 is the fundamental matrix of a pure image shift and every
    twin lies on its line; the poses only give the epipole, which falls inside the image.  The first 40 twins sit within 6 px of it in
    keyframe 2, inside the exclusion radius of every level (10 px at level 0), without map points and with close descriptors: 24 are
    mono on both sides, so only the epipole keeps them from pairing; 16 are stereo on one side or both and are exempt."""
    rng = np.random.default_rng(seed)
    n, n_epi = 360, 40
    sc = Scene(200, rng)                                             # only whether a slot holds a point matters here
    dx, dy = 11.0, -3.0
    f1, f2 = Feats(), Feats()
    order = rng.permutation(n)
    rows = []
    R1, t1 = rot([0, 1, 0], 10.0).astype(F32), np.array([0.05, -0.02, 0.4], F32)
    R2, t2 = rot([1, 0.2, 0], 2.0).astype(F32), np.array([0.02, 0.01, -0.1], F32)
    C2 = R2.astype(F64) @ (-R1.astype(F64).T @ t1.astype(F64)) + t2.astype(F64)
    ex, ey = 500.0 * C2[0] / C2[2] + 319.5, 500.0 * C2[1] / C2[2] + 239.5
    assert 60 < ex < W - 60 and 60 < ey < H - 60
    for i in range(n):
        epi = i < n_epi
        if epi:
            rad, th = rng.uniform(0, 6), rng.uniform(0, 2 * np.pi)
            x, y = ex - dx + rad * np.cos(th), ey - dy + rad * np.sin(th)
            s1, s2 = (False, False) if i < 24 else ((True, False) if i < 29 else ((False, True) if i < 34 else (True, True)))
        else:
            x, y = rng.uniform(30, W - 30), rng.uniform(30, H - 30)
            s1, s2 = rng.random() < 0.5, rng.random() < 0.5
        d = rng.integers(0, 256, 32).astype(np.uint8)
        d[0] = (d[0] & 0x0F) | ((i % 12) << 4)                          # twelve BoW nodes
        a = rng.uniform(0, 360)
        octave = int(rng.integers(0, 8))
        f1.add(x, y, octave, d, right=(x - 5.0 if s1 else -1.0), angle=a, mp=(i % 100 if (not epi and rng.random() < 0.25) else -1))
        rows.append((x, y, octave, d, a, s2, epi))
    for i in order:
        x, y, octave, d, a, s2, epi = rows[i]
        c = rng.random()
        a2 = (a + rng.uniform(0.5, 5)) % 360 if (c < 0.93 or epi) else (a + (120.0 if c < 0.965 else 200.0)) % 360    # one rotation bin, two stray ones
        off_line = (not epi) and rng.random() < 0.1
        far_desc = (not epi) and rng.random() < 0.1
        f2.add(x + dx + rng.uniform(-0.3, 0.3), y + dy + (6.0 * SF[octave] if off_line else rng.uniform(-0.4, 0.4)), octave,
               flip_bits(d, rng.integers(60, 90) if far_desc else rng.integers(0, 30), rng, first_byte=1),
               right=(x + dx - 5.0 if s2 else -1.0), angle=a2, mp=(100 + int(i) % 100 if (not epi and rng.random() < 0.25) else -1))
    sc.add_keyframe(R1, t1, f1)
    sc.add_keyframe(R2, t2, f2)
    sc.link()
    F = np.array([[0, 0, 0], [0, 0, -1], [0, 1, -dy]], F32)
    sc.args = dict(kf1=0, kf2=1, F=F, stereo_only=stereo_only, check_ori=check_ori)
    return sc


def statement_tri(sc, centre="stored"):
    """orbMatcher.cpp:463-470: the epipole is the first keyframe's stored camera centre (-R1^T t1) seen by the second, C2 = R2w Cw + t2w,
    (fx C2x / C2z + cx, fy C2y / C2z + cy); a feature is eligible when its slot in the keyframe holds no map point.  Alternative
    readings: centre = "Rt" takes -R1 t1 for the centre, centre = "swap" projects the second keyframe's centre into the first."""
    k1, k2 = sc.kfs[sc.args["kf1"]], sc.kfs[sc.args["kf2"]]
    if centre == "swap":
        C2 = (gemv32(k1["R"], k2["O"][None])[0] + k1["t"]).astype(F32)
    else:
        Cw = k1["O"] if centre == "stored" else gemv32(-k1["R"], k1["t"])[0]
        C2 = (gemv32(k2["R"], Cw[None])[0] + k2["t"]).astype(F32)
    ex, ey = F32(F32(F32(FX * C2[0]) / C2[2]) + CX), F32(F32(F32(FY * C2[1]) / C2[2]) + CY)
    return dict(epipole=(ex, ey), mp1=(k1["mp_of"] >= 0).astype(np.uint8), mp2=(k2["mp_of"] >= 0).astype(np.uint8))


def double_tri(sc):
    k1, k2 = sc.kfs[sc.args["kf1"]], sc.kfs[sc.args["kf2"]]
    R1, t1, R2, t2 = (a.astype(F64) for a in (k1["R"], k1["t"], k2["R"], k2["t"]))
    C2 = R2 @ (-R1.T @ t1) + t2
    return float(FX) * C2[0] / C2[2] + float(CX), float(FY) * C2[1] / C2[2] + float(CY)


def tri_pairs(sc, search, epipole):
    st = statement_tri(sc)
    k1, k2 = sc.kfs[sc.args["kf1"]], sc.kfs[sc.args["kf2"]]
    return search.triangulation(k1, st["mp1"], k2, st["mp2"], sc.args["F"], epipole, sc.args["stereo_only"], sc.args["check_ori"])


def expected_tri(sc, search):
    """The adapter's result on the statement's epipole and flags; the same search with the epipole far outside the image says which
    pairs the epipole alone removes (mono on both sides, inside the exclusion radius) - none can be when stereoOnly, where both sides
    are stereo and exempt."""
    st = statement_tri(sc)
    k1, k2 = sc.kfs[sc.args["kf1"]], sc.kfs[sc.args["kf2"]]
    n, out = tri_pairs(sc, search, st["epipole"])
    _, free = tri_pairs(sc, search, (F32(-1.0e4), F32(-1.0e4)))
    first = np.flatnonzero(out >= 0)
    pairs = np.stack([first, out[first]], axis=1).astype(np.int32).reshape(-1)
    ex, ey = st["epipole"]
    near = lambda k, i: (float(ex) - float(k["kps"]["x"][i])) ** 2 + (float(ey) - float(k["kps"]["y"][i])) ** 2 < 100.0 * float(SF[k["kps"]["octave"][i]])
    counts = dict(matches=int(n), has_point_1=int(st["mp1"].sum()), has_point_2=int(st["mp2"].sum()),
                  near_epipole_2=int(sum(1 for i in range(len(k2["kps"])) if near(k2, i))),
                  removed_by_epipole=int(((free >= 0) & (out < 0)).sum()), changed_by_epipole=int((free != out).sum()),
                  near_epipole_exempt=int(sum(1 for i in first if near(k2, out[i]) and (k1["right"][i] >= 0 or k2["right"][out[i]] >= 0))),
                  mono_pairs=int(sum(1 for i in first if k1["right"][i] < 0 and k2["right"][out[i]] < 0)))
    return n, pairs, State(sc), counts


def blob_tri(sc):
    a = sc.args
    return sc.world_blob() + struct.pack("<2i", a["kf1"], a["kf2"]) + a["F"].tobytes() + struct.pack("<2i", int(a["stereo_only"]), int(a["check_ori"]))


# =================================================================================================================================
# What the tests iterate over
# =================================================================================================================================
CASES = {
    "mappoint": (scenario_mappoint, expected_mappoint, blob_mappoint),
    "reloc": (scenario_reloc, expected_reloc, blob_reloc),
    "sim": (scenario_sim, expected_sim, blob_sim),
    "sim3": (scenario_sim3, expected_sim3, blob_sim3),
    "fuse": (scenario_fuse, expected_fuse, blob_fuse),
    "fusesim": (scenario_fusesim, expected_fusesim, blob_fusesim),
    "tri": (scenario_tri, expected_tri, blob_tri),
}
# every branch an adapter's scenario has to show at least three times (and at least ten accepted matches)
BRANCHES = {
    "mappoint": ("not_in_view", "bad", "level0", "level7", "level0_matched", "level7_matched", "stereo_matched", "observed", "unobserved", "radius_2_5",
                 "radius_4_0", "prefilled_taken", "prefilled_free_overwritten"),
    "reloc": ("culled", "found_skipped", "null", "bad", "behind", "outside", "too_close", "too_far", "taken_any", "taken_unobserved"),
    "reloc_no_ori": ("found_skipped", "null", "bad", "behind", "outside", "too_close", "too_far", "taken_any", "taken_unobserved"),
    "sim": ("prefilled", "found_skipped", "found_would_match", "null", "bad", "behind", "outside", "invariance", "angle"),
    "sim3": ("one_way", "done1", "done2", "absent_from_kf2", "one_way_because_done2", "rejected12", "rejected21"),
    "fuse": ("added", "held_more", "held_fewer", "held_equal", "bad_held", "bad_at_turn", "in_kf_at_turn", "in_kf_before", "stereo_feature", "mono_feature",
             "null", "behind", "outside", "too_close", "too_far", "angle"),
    "fusesim": ("added", "replaced", "bad_held", "self_again", "bad_at_turn", "found_skipped", "stereo_feature", "rejected", "null"),
    "tri": ("has_point_1", "has_point_2", "near_epipole_2", "removed_by_epipole", "near_epipole_exempt", "mono_pairs"),
    "tri_stereo_only": ("has_point_1", "has_point_2", "near_epipole_2", "near_epipole_exempt"),     # both sides stereo: nothing the epipole can remove
}


def check_counts(name, counts):
    assert counts["matches"] >= 10, (name, counts)
    for k in BRANCHES[name]:
        assert counts[k] >= 3, (name, k, counts)


# =================================================================================================================================
# stereo: Frame::computeStereoMatches (frame.cpp:362-477) through computeStereoMatchesImpl of include/ydorb/frame.hpp
# =================================================================================================================================
STEREO_W, STEREO_H, STEREO_NF, STEREO_INDEX = 320, 240, 300, 6
STEREO_B, STEREO_BF = F32(0.1), F32(40.0)


def stereo_pair():
    from ydorbslam_amd.synth import synth_stereo_pair
    left, right, _ = synth_stereo_pair(STEREO_W, STEREO_H, STEREO_INDEX)
    return np.ascontiguousarray(left), np.ascontiguousarray(right)


def stereo_oracle(oracle_lib, by_kp, left=None, right=None):
    """The CPU restatement on the pair: extraction, then stereo matching over the extractor's own pyramids."""
    if left is None:
        left, right = stereo_pair()
    el, er = oracle_lib.OrbExtractorOracle(STEREO_NF), oracle_lib.OrbExtractorOracle(STEREO_NF)
    kl, dl = el.extract(left)
    kr, dr = er.extract(right)
    lv_l = [el.level_padded(l)[19:19 + el.level_dims(l)[1], 19:19 + el.level_dims(l)[0]] for l in range(8)]
    lv_r = [er.level_padded(l)[19:19 + er.level_dims(l)[1], 19:19 + er.level_dims(l)[0]] for l in range(8)]
    t = el.tables()
    rx, depth, kept, status = oracle_lib.stereo_matches(kl, dl, kr, dr, lv_l, lv_r, t["scale"], t["inv_scale"], float(STEREO_BF), float(STEREO_B), by_kp)
    return dict(kl=kl, dl=dl, kr=kr, dr=dr, rx=rx, depth=depth, kept=int(kept), status=int(status))


def blob_stereo(left, right, flags, variant):
    return struct.pack("<5i2f", STEREO_W, STEREO_H, STEREO_NF, flags, variant, STEREO_B, STEREO_BF) + left.tobytes() + right.tobytes()


def parse_stereo(out):
    threw, status, n = struct.unpack_from("<3i", out, 0)
    off = 12
    rx = np.frombuffer(out, np.uint32, n, off); off += 4 * n
    nd = struct.unpack_from("<i", out, off)[0]; off += 4
    depth = np.frombuffer(out, np.uint32, nd, off); off += 4 * nd
    sides = []
    for _ in range(2):
        m = struct.unpack_from("<i", out, off)[0]; off += 4
        kps = np.frombuffer(out, KP_DTYPE, m, off); off += 28 * m
        desc = np.frombuffer(out, np.uint8, 32 * m, off).reshape(m, 32); off += 32 * m
        sides.append((kps, desc))
    assert off == len(out)
    return dict(threw=threw, status=status, rx=rx, depth=depth, left=sides[0], right=sides[1])
