"""Test support of ydorb_mapdb_local_ba_graph: seeded scenes, the CPU restatement of the sequential loops
(tests/localba_ref/localba_ref.cpp, built with the flags of the other references), a second statement of the contract in Python dicts,
and the loading of a scene into a MapDb.  Every comparison is exact; doubles are compared by bit pattern."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from mapmaint_support import ROOT, _flags
from ydorbslam_amd.extractor import KP_DTYPE

REF_SRC = os.path.join(ROOT, "tests", "localba_ref", "localba_ref.cpp")
CHECK_SRC = os.path.join(ROOT, "tests", "cpu_harness", "mapdb_lba_check.cpp")
SKIPPED_VIEWS, VIEW_OUT_OF_RANGE, NO_EDGES = 1, 2, 4
SIGMA = np.array([1.0 / np.float32(1.2) ** (2 * l) for l in range(8)], np.float32)   # m_v_invScaleFactorSquares of the default pyramid
GRAPH_KEYS = ("pose_kf", "pose_fixed", "point_slot", "point_status", "points", "edge_pose", "edge_point", "edge_kf", "edge_idx", "edge_meas", "edge_inv_sigma2")
_REF = None
_VP, _I = C.c_void_p, C.c_int32


def _p(a):
    return a.ctypes.data_as(_VP) if a is not None else None


def _csr(lists, dtype):
    start = np.concatenate([[0], np.cumsum([len(a) for a in lists])]).astype(np.int32)
    return start, np.ascontiguousarray(np.concatenate([np.asarray(a, dtype).reshape(-1) for a in lists] + [np.zeros(0, dtype)]))


class Scene:
    """A map as the resident table holds it: rows [n_kf] of point slots, views [n_points] of (kf, idx), feats [n_kf] of (kps, right_x),
    bad [n_points], pos [n_points, 3].  Keyframes 0 .. n_local-1 are the local ones of the default call.

    The default: 6 local keyframes of 300 features, 40 others of 140 and 39 sparse ones of 4 that only the 70-view point sees, 760 points
    of which 700 lie in local rows; spans of 1 to 12 views in a shuffled order; others 30..34 are seen only by points whose first local
    observer is keyframe 3 or later and others 35..39 only by points that keyframe 5 alone sees, so their first occurrence has a high rank;
    three others have no features (culled); every third keyframe is monocular."""

    def __init__(self, seed=1, n_local=6, n_other=40, n_sparse=39, n_local_points=700, n_far_points=60, local_feats=300, other_feats=140, max_span=12,
                 big_views=70, mono_all=False, late=10):
        r = np.random.default_rng(seed)
        self.n_local, self.n_kf, self.n_points = n_local, n_local + n_other + n_sparse, n_local_points + n_far_points
        others = np.arange(n_local, n_local + n_other)
        sparse = np.arange(n_local + n_other, self.n_kf)
        n_feat = np.array([local_feats] * n_local + [other_feats] * n_other + [4] * n_sparse)
        perm = [r.permutation(n) for n in n_feat]
        used = np.zeros(self.n_kf, np.int64)
        self.rows = [np.full(n, -1, np.int32) for n in n_feat]
        self.views = []
        half = late // 2
        for p in range(self.n_points):
            if p < n_local_points:
                loc = np.sort(r.choice(n_local, size=int(r.integers(1, min(3, n_local) + 1)), replace=False))
            else:
                loc = np.zeros(0, np.int64)
            allowed = n_other - late                         # the others before the late groups
            if len(loc) and loc.min() >= n_local // 2:
                allowed = n_other - half
            if len(loc) and loc.min() == n_local - 1:
                allowed = n_other
            if not len(loc):
                allowed = n_other - late
            want = int(r.integers(1, max_span + 1))
            oth = others[r.choice(allowed, size=min(max(want - len(loc), 0), allowed), replace=False)] if allowed > 0 else np.zeros(0, np.int64)
            obs = np.concatenate([loc, oth]).astype(np.int64)
            if p == 5 and big_views:                           # more views than a wave has lanes; the sparse keyframes come last
                pick = others[r.permutation(allowed)[:big_views - 1 - n_sparse]]
                obs = np.concatenate([r.permutation(np.concatenate([[0], pick])), sparse])
            elif len(obs):
                obs = r.permutation(obs)
            obs = np.array([k for k in obs if used[k] < n_feat[k]], np.int64)
            v = np.zeros((len(obs), 2), np.int32)
            for j, k in enumerate(obs):
                idx = perm[k][used[k]]
                used[k] += 1
                v[j] = (k, idx)
                self.rows[k][idx] = p
            self.views.append(v)
        self.bad = np.zeros(self.n_points, np.uint8)
        self.bad[r.choice(self.n_points, size=max(self.n_points // 35, 1), replace=False)] = 1
        self.bad[5] = 0
        self.pos = r.normal(size=(self.n_points, 3)).astype(np.float32) * 3
        self.feats = []
        for k, n in enumerate(n_feat):
            kp = np.zeros(n, KP_DTYPE)
            kp["x"], kp["y"] = r.uniform(0, 640, n).astype(np.float32), r.uniform(0, 480, n).astype(np.float32)
            kp["size"], kp["angle"], kp["response"], kp["class_id"] = 31, r.uniform(0, 360, n).astype(np.float32), 20, -1
            kp["octave"] = r.integers(0, 8, n)
            rx = np.where(r.random(n) < 0.6, kp["x"] - r.uniform(1, 40, n), -1).astype(np.float32)
            if mono_all or k % 3 == 2:
                rx[:] = -1
            self.feats.append((kp, rx))
        self.mono_all = mono_all
        if n_local_points > 40:
            self.views[40] = np.zeros((0, 2), np.int32)      # a point in a local row that nobody is recorded to see
        for k in others[[3, 11, 17]] if n_other > 17 else others[:1]:      # culled keyframes: still named by views
            self.feats[k] = (np.zeros(0, KP_DTYPE), np.zeros(0, np.float32))
        self.kf_slots = np.arange(n_local, dtype=np.int32)

    def load(self, db, features=True):
        if features:
            db.enable_features()
        db.set_centres(np.arange(self.n_kf), np.zeros((self.n_kf, 3), np.float32))
        n = self.n_points
        db.set_points(np.arange(n), [v[:, 0] for v in self.views], [np.zeros(len(v), np.uint8) for v in self.views], self.bad, np.zeros(n, np.int32),
                      np.zeros(n, np.uint8), self.pos)
        db.set_keyframe_rows(np.arange(self.n_kf), self.rows)
        db.set_point_views(np.arange(n), self.views)
        if features:
            db.set_keyframe_features(np.arange(self.n_kf), [f[0] for f in self.feats], None if self.mono_all else [f[1] for f in self.feats])
        return db

    def tables(self):
        return dict(rows=self.rows, views=self.views, feats=self.feats, bad=self.bad, pos=self.pos)


def exported(db):
    """The tables of a handle read back through its exports, in the form Scene.tables() has."""
    e = db.export()
    return dict(rows=db.export_rows(), views=db.export_views(), feats=db.export_features(), bad=e["table"].bad, pos=e["pos"])


def ref():
    global _REF
    if _REF is None:
        out = os.path.join(tempfile.mkdtemp(prefix="localbaref"), "liblocalbaref.so")
        subprocess.check_call(["g++", *_flags(), "-shared", "-o", out, REF_SRC])
        L = C.CDLL(out)
        L.localbaref_graph.restype = C.c_int
        L.localbaref_graph.argtypes = [_I, _I] + [_VP] * 11 + [_I] + [_VP] * 13
        _REF = L
    return _REF


def ref_inputs(t):
    """The flat arrays of tables `t` (Scene.tables() or exported()) as the restatement takes them, and room for its outputs."""
    n_kf, n_pts = len(t["rows"]), len(t["bad"])
    row_start, row_slot = _csr(t["rows"], np.int32)
    views = list(t["views"]) + [np.zeros((0, 2), np.int32)] * (n_pts - len(t["views"]))
    view_start = np.concatenate([[0], np.cumsum([len(v) for v in views])]).astype(np.int32)
    flat = np.concatenate([np.asarray(v, np.int32).reshape(-1, 2) for v in views] + [np.zeros((0, 2), np.int32)])
    view_kf, view_idx = np.ascontiguousarray(flat[:, 0]), np.ascontiguousarray(flat[:, 1])
    feat_start = np.concatenate([[0], np.cumsum([len(f[0]) for f in t["feats"]])]).astype(np.int32)
    kps = np.ascontiguousarray(np.concatenate([f[0] for f in t["feats"]] + [np.zeros(0, KP_DTYPE)]))
    rx = np.ascontiguousarray(np.concatenate([np.asarray(f[1], np.float32) for f in t["feats"]] + [np.zeros(0, np.float32)]))
    bad, pos = np.ascontiguousarray(t["bad"], np.uint8), np.ascontiguousarray(t["pos"], np.float32)
    K, P, E = max(n_kf, 1), max(n_pts, 1), max(len(view_kf), 1)
    o = dict(pose_kf=np.zeros(K, np.int32), pose_fixed=np.zeros(K, np.uint8), point_slot=np.zeros(P, np.int32), point_status=np.zeros(P, np.uint8),
             points=np.zeros((P, 3)), edge_pose=np.zeros(E, np.int32), edge_point=np.zeros(E, np.int32), edge_kf=np.zeros(E, np.int32),
             edge_idx=np.zeros(E, np.int32), edge_meas=np.zeros((E, 3)), edge_inv_sigma2=np.zeros(E))
    return dict(n_kf=n_kf, n_pts=n_pts, arrays=(row_start, row_slot, bad, pos, view_start, view_kf, view_idx, feat_start, kps, rx), out=o, counts=np.zeros(4, np.int32))


def ref_run(inp, kf_slots, sigma=SIGMA):
    """One call of the restatement on prepared inputs: the part a timing measures.  Returns the counts."""
    kf = np.ascontiguousarray(kf_slots, np.int32).reshape(-1)
    sig = np.ascontiguousarray(sigma, np.float32)
    o = inp["out"]
    rc = ref().localbaref_graph(inp["n_kf"], inp["n_pts"], *[_p(a) for a in inp["arrays"]], _p(kf), len(kf), _p(sig), _p(inp["counts"]), _p(o["pose_kf"]),
                                _p(o["pose_fixed"]), _p(o["point_slot"]), _p(o["point_status"]), _p(o["points"]), _p(o["edge_pose"]), _p(o["edge_point"]),
                                _p(o["edge_kf"]), _p(o["edge_idx"]), _p(o["edge_meas"]), _p(o["edge_inv_sigma2"]))
    assert rc == 0
    return inp["counts"]


def ref_graph(t, kf_slots, sigma=SIGMA):
    """The reference restatement on tables `t` (Scene.tables() or exported()).  Returns the dict MapDb.local_ba_graph returns."""
    inp = ref_inputs(t)
    nl, nf, npts, ne = (int(c) for c in ref_run(inp, kf_slots, sigma))
    size = dict(pose_kf=nl + nf, pose_fixed=nl + nf, point_slot=npts, point_status=npts, points=npts)
    out = {k: v[:size.get(k, ne)].copy() for k, v in inp["out"].items()}
    out.update(n_local=nl, n_fixed=nf)
    return out


def dict_graph(t, kf_slots, sigma=SIGMA):
    """The contract stated a second time, with Python dicts and lists and none of the reference's tags."""
    kf_slots = [int(k) for k in np.asarray(kf_slots).reshape(-1)]
    sigma = np.asarray(sigma, np.float32)
    n_feat = {k: len(f[0]) for k, f in enumerate(t["feats"])}
    pose_of = {k: i for i, k in enumerate(kf_slots)}
    local_points = list(dict.fromkeys(int(s) for k in kf_slots for s in t["rows"][k] if s >= 0 and not t["bad"][s]))
    views = lambda s: [(int(k), int(i)) for k, i in t["views"][s]] if s < len(t["views"]) else []
    fixed = list(dict.fromkeys(k for s in local_points for k, i in views(s) if n_feat.get(k, 0) > 0 and k not in pose_of))
    pose_kf = kf_slots + fixed
    pose_of.update({k: len(kf_slots) + j for j, k in enumerate(fixed)})
    ep, eq, ek, ei, meas, info, status = [], [], [], [], [], [], []
    for p, s in enumerate(local_points):
        st, n0 = 0, len(ep)
        for k, i in views(s):
            if n_feat.get(k, 0) == 0:
                st |= SKIPPED_VIEWS
            elif i >= n_feat[k]:
                st |= VIEW_OUT_OF_RANGE
            else:
                kp, ur = t["feats"][k][0][i], np.float32(t["feats"][k][1][i])
                ep.append(pose_of[k]); eq.append(p); ek.append(k); ei.append(i)
                meas.append((np.float64(kp["x"]), np.float64(kp["y"]), np.float64(-1.0) if ur < 0 else np.float64(ur)))
                info.append(np.float64(sigma[kp["octave"]]))
        status.append(st | (NO_EDGES if len(ep) == n0 else 0))
    i32 = lambda a: np.array(a, np.int32).reshape(-1)
    return dict(n_local=len(kf_slots), n_fixed=len(fixed), pose_kf=i32(pose_kf), pose_fixed=np.array([0] * len(kf_slots) + [1] * len(fixed), np.uint8),
                point_slot=i32(local_points), point_status=np.array(status, np.uint8).reshape(-1),
                points=np.asarray(t["pos"], np.float32)[local_points].astype(np.float64).reshape(-1, 3), edge_pose=i32(ep), edge_point=i32(eq),
                edge_kf=i32(ek), edge_idx=i32(ei), edge_meas=np.array(meas, np.float64).reshape(-1, 3), edge_inv_sigma2=np.array(info, np.float64).reshape(-1))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same_graph(got, want):
    """Counts and every array, exactly."""
    assert (got["n_local"], got["n_fixed"]) == (want["n_local"], want["n_fixed"]), (got["n_local"], got["n_fixed"], want["n_local"], want["n_fixed"])
    for k in GRAPH_KEYS:
        assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        assert got[k].dtype == want[k].dtype, (k, got[k].dtype, want[k].dtype)
        assert np.array_equal(bits(got[k]), bits(want[k])), k


def first_occurrence(g):
    """Per fixed keyframe of a graph, where its first edge lies: (rank of the point, position of the edge among that point's edges)."""
    out = {}
    start = np.searchsorted(g["edge_point"], np.arange(len(g["point_slot"])))
    for e in range(len(g["edge_pose"])):
        k = int(g["edge_kf"][e])
        if g["edge_pose"][e] >= g["n_local"] and k not in out:
            out[k] = (int(g["edge_point"][e]), e - int(start[g["edge_point"][e]]))
    return out


def make_geometric(scene, seed=3, camera=(500.0, 500.0, 320.0, 240.0, 40.0), noise=0.5):
    """Replaces positions and measurements of a scene by a consistent geometry, so that a solve on its graph converges: keyframes along
    x looking down z, points in front of them.  Returns (poses [n_kf, 7] of every keyframe slot, perturbed from the truth; camera)."""
    r = np.random.default_rng(seed)
    fx, fy, cx, cy, bf = camera
    t = np.zeros((scene.n_kf, 3))
    t[:, 0] = -0.25 * np.arange(scene.n_kf)
    scene.pos = np.stack([r.uniform(-2, 5, scene.n_points), r.uniform(-2, 2, scene.n_points), r.uniform(5, 11, scene.n_points)], axis=1).astype(np.float32)
    for p, v in enumerate(scene.views):
        for k, i in v:
            kp, rx = scene.feats[k]
            if i >= len(kp):
                continue
            xc = scene.pos[p].astype(np.float64) + t[k]
            u, w = fx * xc[0] / xc[2] + cx + r.normal() * noise, fy * xc[1] / xc[2] + cy + r.normal() * noise
            kp["x"][i], kp["y"][i] = u, w
            if rx[i] >= 0:
                rx[i] = np.float32(u - bf / xc[2])
    poses = np.zeros((scene.n_kf, 7))
    poses[:, :3] = t + r.normal(size=t.shape) * 0.01
    poses[:, 6] = 1.0
    scene.pos = (scene.pos + r.normal(size=scene.pos.shape).astype(np.float32) * np.float32(0.02)).astype(np.float32)
    return poses, np.array(camera)


def solver_scene():
    """Sized for the solver's smallest interesting case: 8 local keyframes, 6 others of which one is culled, about 300 points, with a
    consistent geometry.  Returns (scene, poses [n_kf, 7], camera [5])."""
    s = Scene(seed=4, n_local=8, n_other=6, n_sparse=0, n_local_points=300, n_far_points=0, local_feats=160, other_feats=320, max_span=8, big_views=0, late=0)
    poses, camera = make_geometric(s)
    return s, poses, camera


def problem_of(g, poses, camera):
    """The dict Optimizer.local_bundle_adjust takes, from a graph and the poses [n_poses, 7] of its keyframes."""
    return dict(poses=np.asarray(poses, np.float64), fixed=g["pose_fixed"], points=g["points"], edge_pose=g["edge_pose"], edge_point=g["edge_point"],
                meas=g["edge_meas"], info=g["edge_inv_sigma2"], camera=camera)
