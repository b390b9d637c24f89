"""Test support of ydorb_mapdb_create_new_points: the reference and the scenes.
The reference is the sequential loop of createNewMapPointsImpl restated on the CPU: per neighbour the matcher oracle's
search_for_triangulation, then the CPU restatement of the geometry (tests/triangulate_ref), with the claim mask carried from
neighbour to neighbour.  The scene builder makes a current keyframe and its neighbours that see the same points (the construction
of tests/test_triangulate_adapter_gpu.py: no pixel noise, since the reference's epipolar test passes only residuals of a few
thousandths of a pixel) and asserts, on the reference alone, that the scene can tell a wrong implementation from a right one."""
import os

import numpy as np

import triangulate_support as S
from triangulate_support import ROOT

f32 = np.float32
CHECK_SRC = os.path.join(ROOT, "tests", "cpu_harness", "mapdb_bow_check.cpp")
UNMATCHED = 15
NB_STATUS = {"ok": 0, "no_features": 1, "no_block": 2, "no_bow": 3, "length_mismatch": 4, "bow_index": 5}
POOL_PER_NEIGHBOUR = 1 << 14   # the records a fresh matcher holds per neighbour (c_api.h): more than that forces the replay


def _mul3(A, B):
    """3x3 float product in the adapter's loops: s = 0; s = s + a * b in ascending k, every operation rounded to float."""
    C = np.zeros((3, B.shape[1]), f32)
    for r in range(3):
        for c in range(B.shape[1]):
            s = f32(0)
            for k in range(3):
                s = f32(s + f32(A[r, k] * B[k, c]))
            C[r, c] = s
    return C


def f12(v1, v2):
    """computeF12 of include/ydorb/localMapping.hpp, operation for operation."""
    R1, t1, R2, t2 = v1["Tcw"][:, :3], v1["Tcw"][:, 3], v2["Tcw"][:, :3], v2["Tcw"][:, 3]
    R12 = _mul3(R1, np.ascontiguousarray(R2.T))
    t12 = (-_mul3(R12, t2.reshape(3, 1))[:, 0] + t1).astype(f32)
    z = f32(0)
    tx = np.array([[z, -t12[2], t12[1]], [t12[2], z, -t12[0]], [-t12[1], t12[0], z]], f32)
    ifx, ify = f32(1) / v1["fx"], f32(1) / v1["fy"]
    Kinv = np.array([[ifx, z, f32(-v1["cx"] * ifx)], [z, ify, f32(-v1["cy"] * ify)], [z, z, f32(1)]], f32)
    return _mul3(_mul3(_mul3(np.ascontiguousarray(Kinv.T), tx), R12), Kinv)


def epipole(v1, v2):
    C2 = (_mul3(v2["Tcw"][:, :3], v1["Ow"].reshape(3, 1))[:, 0] + v2["Tcw"][:, 3]).astype(f32)
    return f32(f32(f32(v1["fx"] * C2[0]) / C2[2]) + v1["cx"]), f32(f32(f32(v1["fy"] * C2[1]) / C2[2]) + v1["cy"])


def default_nodes(point, kf):
    return (point % 12).astype(np.uint32) * 5 + 2   # 12 vocabulary nodes, ids not contiguous


def bucket_nodes(point, kf):
    """Buckets of exactly 130 (three gather rounds), 64 and 65 features in every keyframe, the rest spread over five nodes."""
    return np.where(point < 130, 10, np.where(point < 194, 20, np.where(point < 259, 30, 40 + point % 5))).astype(np.uint32)


def end_nodes(point, kf):
    """The first keyframe files a twelfth of its features under a node below every node of the neighbours and another twelfth under a
    node above them all: the two ends of the join's binary search."""
    base = default_nodes(point, kf)
    if kf == 0:
        base = np.where(point % 12 == 0, 1, np.where(point % 12 == 11, 999983, base)).astype(np.uint32)
    return base


def one_node(point, kf):
    return np.full(len(point), 77, np.uint32)


class Scene:
    """kfs[0] is the first keyframe, kfs[1:] the neighbours in order.  Each: view (triangulate.make_view), desc [n, 32], nodes [n], bow
    [n, 2] (node, feature) in map order, fv (the oracle's CSR triple), row [n] point slot or -1.  slots[k] = the keyframe's slot."""

    def __init__(self, seed=5, n=300, n_nb=4, nodes=default_nodes, mapped=0.15, extra=7, disjoint=(), poses=None, seen=0.42):
        from ydorbslam_amd import KP_DTYPE
        from ydorbslam_amd.triangulate import make_view
        rng = np.random.default_rng(seed)
        poses = poses or [S.pose(), S.pose(S.rot((0.1, 1, 0.05), np.radians(3.0)), (0.45, 0.03, 0.05)), S.pose(S.rot((0, 1, 0.1), np.radians(-2.5)), (-0.4, 0.02, 0.0)),
                 S.pose(S.rot((1, 0.2, 0), np.radians(2.0)), (0.05, -0.42, 0.03)), S.pose(S.rot((0.3, 1, 0), np.radians(-3.5)), (0.38, 0.3, -0.05)),
                 S.pose(S.rot((0, 1, 0), np.radians(1.5)), (-0.3, -0.3, 0.02))]
        assert n_nb + 1 <= len(poses)
        z = rng.uniform(1.5, 10.0, n)
        X = np.stack([rng.uniform(-0.3, 0.3, n) * z, rng.uniform(-0.22, 0.22, n) * z, z], axis=1)
        base = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        octave = rng.integers(0, 8, n)
        angle = rng.uniform(0, 360, n)
        self.n_points = 64                                   # the map points the rows name
        self.kfs, self.slots = [], [int(s) for s in rng.permutation(n_nb + 3)[:n_nb + 1]]
        for k in range(n_nb + 1):
            m = n + (extra * k if k else 0)                  # the neighbours hold a few features more, of no point
            order = np.concatenate([rng.permutation(n), n + np.arange(m - n)])
            real = order < n
            seen_k = real & (rng.uniform(size=m) < (1.0 if k == 0 else seen))   # a neighbour sees two fifths of the points: the later ones keep some to match
            uv, d = np.zeros((m, 2)), np.ones(m)
            uv[real], d[real] = S.project(poses[k], X[order[real]])
            uv[~seen_k] = rng.uniform(20, 460, (int((~seen_k).sum()), 2))
            kps = np.zeros(m, KP_DTYPE)
            kps["x"], kps["y"], kps["class_id"], kps["size"] = uv[:, 0], uv[:, 1], -1, 31
            kps["octave"] = np.where(real, octave[np.minimum(order, n - 1)], 0)
            if k == 1:                                        # a fifth of neighbour 0's features four levels off: the scale test rejects them
                off = rng.uniform(size=m) < 0.2
                kps["octave"] = np.where(off, (kps["octave"] + 4) % 8, kps["octave"])
            turn = np.where(rng.uniform(size=m) < 0.85, 10.0 * k, rng.uniform(0, 360, m))   # most features turn with the keyframe
            kps["angle"] = (np.where(real, angle[np.minimum(order, n - 1)], 0.0) + turn) % 360.0
            stereo = rng.uniform(size=m) < 0.5
            right = np.where(stereo, uv[:, 0] - S.BF / d + rng.normal(0, 0.5, m), -1.0).astype(f32)
            depth = np.where(stereo, d, -1.0).astype(f32)
            desc = rng.integers(0, 256, (m, 32), dtype=np.uint8)
            desc[seen_k] = base[order[seen_k]]
            for r in np.flatnonzero(seen_k):
                for bit in rng.integers(0, 256, 3):
                    desc[r, bit // 8] ^= np.uint8(1 << (bit % 8))
            nd = nodes(order.astype(np.int64), k).astype(np.uint32)
            if k in disjoint:
                nd = nd + np.uint32(5000)
            row = np.where(rng.uniform(size=m) < mapped, rng.integers(0, self.n_points, m), -1).astype(np.int32)
            self.kfs.append(self._keyframe(make_view(kps, right, depth, poses[k], S.K, S.B, S.BF), desc, nd, row))

    @staticmethod
    def _keyframe(view, desc, nodes, row):
        from helpers import feature_vector
        fv = feature_vector(nodes)
        bow = np.stack([np.repeat(fv[0].astype(np.int64), np.diff(fv[1])), fv[2].astype(np.int64)], axis=1)
        return dict(view=view, desc=np.ascontiguousarray(desc), nodes=nodes, fv=fv, bow=bow, row=row)

    @property
    def n(self):
        return len(self.kfs[0]["row"])

    @property
    def n_nb(self):
        return len(self.kfs) - 1

    # -------------------------------------------------------------------------------------------------- the resident table
    def load(self, db, skip=()):
        """Puts the scene into a MapDb; the relations named in `skip` ("rows", "blocks", "features", "bow") stay out."""
        db.enable_features()
        db.enable_bow()
        P = self.n_points
        db.set_centres(np.arange(max(self.slots) + 1), np.zeros((max(self.slots) + 1, 3), f32))   # the keyframes exist before a point names one
        db.set_points(np.arange(P), [[] for _ in range(P)], [[] for _ in range(P)], np.zeros(P, np.uint8), np.zeros(P, np.int32), np.zeros(P, np.uint8),
                      np.zeros((P, 3), f32))
        if "rows" not in skip:
            db.set_keyframe_rows(self.slots, [k["row"] for k in self.kfs])
        if "blocks" not in skip:
            db.set_keyframe_descriptors(self.slots, [k["desc"] for k in self.kfs])
        if "features" not in skip:
            db.set_keyframe_features(self.slots, [k["view"]["kps"] for k in self.kfs], [k["view"]["right_x"] for k in self.kfs])
        if "bow" not in skip:
            db.set_keyframe_bow(self.slots, [k["bow"] for k in self.kfs])

    def call(self, order=None):
        """(first, neighbours, keep): the structs of MapDb.create_new_points for the neighbours `order` (indices into kfs, default all)."""
        from ydorbslam_amd.map_resident import create_neighbour, create_view
        order = list(range(1, len(self.kfs))) if order is None else list(order)
        keep = []

        def view(k):
            v = self.kfs[k]["view"]
            cv, depth = create_view(self.slots[k], v["depth"], v["Tcw"], v["Ow"], float(v["fx"]), float(v["fy"]), float(v["cx"]), float(v["cy"]),
                                    float(v["b"]), float(v["bf"]), v["level_sigma2"], v["scale_factors"])
            keep.append(depth)
            return cv
        v1 = self.kfs[0]["view"]
        rf = float(f32(1.5) * v1["scale_factors"][1])
        nbs = []
        for k in order:
            ex, ey = epipole(v1, self.kfs[k]["view"])
            nbs.append(create_neighbour(view(k), f12(v1, self.kfs[k]["view"]), float(ex), float(ey), rf))
        return view(0), nbs, keep

    # -------------------------------------------------------------------------------------------------- the reference
    def reference(self, oracle, order=None, stereo_only=False, check_orientation=False, claims=True):
        """The sequential loop on the CPU.  Returns the dict of MapDb.create_new_points (without neighbour_status)."""
        order = list(range(1, len(self.kfs))) if order is None else list(order)
        A, n = self.kfs[0], self.n
        v1 = A["view"]
        has0 = (A["row"] >= 0).astype(np.uint8)
        claimed = np.zeros(n, np.uint8)
        out = dict(matched_second=np.full((len(order), n), -1, np.int32), x3d=np.zeros((len(order), n, 3), f32),
                   status=np.full((len(order), n), UNMATCHED, np.uint8), n_matches=np.zeros(len(order), np.int32), n_accepted=np.zeros(len(order), np.int32))
        for i, k in enumerate(order):
            B = self.kfs[k]
            v2 = B["view"]
            has_a = (has0 | claimed) if claims else has0
            n_m, match = oracle.search_for_triangulation(v1["kps"], A["desc"], has_a, v1["right_x"], A["fv"], v2["kps"], B["desc"], (B["row"] >= 0).astype(np.uint8),
                                                         v2["right_x"], B["fv"], f12(v1, v2), epipole(v1, v2), v2["scale_factors"], v2["level_sigma2"],
                                                         stereo_only, check_orientation)
            i1 = np.flatnonzero(match >= 0).astype(np.int32)
            assert n_m == len(i1)
            out["n_matches"][i] = n_m
            if n_m == 0:
                continue
            r = S.ref_triangulate([v1, v2], [dict(first=0, second=1, idx1=i1, idx2=match[i1])])[0]
            out["matched_second"][i, i1], out["x3d"][i, i1], out["status"][i, i1] = match[i1], r["x3d"], r["status"]
            acc = (r["status"] & 15) == 0
            out["n_accepted"][i] = int(acc.sum())
            claimed[i1[acc]] = 1
        return out


def assert_same(got, want):
    """All five outputs, exactly; positions by bit pattern."""
    assert np.array_equal(got["n_matches"], want["n_matches"]), (got["n_matches"], want["n_matches"])
    assert np.array_equal(got["matched_second"], want["matched_second"])
    assert np.array_equal(got["status"], want["status"])
    assert np.array_equal(got["x3d"].view(np.uint32), want["x3d"].view(np.uint32))
    assert np.array_equal(got["n_accepted"], want["n_accepted"])


def check_scene_conditions(scene, oracle):
    """Conditions on the inputs, stated on the reference alone.  Returns (with claims, without claims)."""
    with_claims = scene.reference(oracle)
    without = scene.reference(oracle, claims=False)
    assert (with_claims["n_matches"] >= 20).all() and (with_claims["n_accepted"] >= 5).all(), (with_claims["n_matches"], with_claims["n_accepted"])
    # the claim rule decides something: a later neighbour's matches differ when the claims are left out
    assert any(not np.array_equal(with_claims["matched_second"][i], without["matched_second"][i]) for i in range(1, scene.n_nb))
    # an idx1 matched and rejected by the geometry with neighbour j is matched again with a later one: a rejection must not claim
    m, st = with_claims["matched_second"], with_claims["status"]
    again = 0
    for j in range(scene.n_nb - 1):
        rejected = (m[j] >= 0) & ((st[j] & 15) != 0)
        again += int((rejected & (m[j + 1:] >= 0).any(axis=0)).sum())
    assert again >= 1
    return with_claims, without


_DEFAULT = None


def default_scene():
    """The default scene, built once: about 300 features, 4 neighbours, 12 vocabulary nodes, a stereo / mono mix, map points on both sides."""
    global _DEFAULT
    if _DEFAULT is None:
        _DEFAULT = Scene()
    return _DEFAULT


# ------------------------------------------------------------------------------------------------------------ the harness' sequence
def parse_trace(lines):
    names = ("round", "n_entries", "pool_used", "pool_capacity", "repacks_kept", "repacks_grown", "last_bow_sync_bytes", "last_bow_sync_records")
    return [dict(zip(names, (int(v) for v in ln.split()[1:]))) for ln in lines]


def read_ops(path):
    """The operations file of mapdb_bow_check: ("set", slots, bows) / ("sync", trace) / ("clear",) in order."""
    ops, lines, i = [], open(path).read().splitlines(), 0
    while i < len(lines):
        t = lines[i].split()
        if t[0] == "B":
            slots, bows = [], []
            for ln in lines[i + 1:i + 1 + int(t[1])]:
                v = [int(x) for x in ln.split()]
                slots.append(v[0])
                bows.append(np.array(v[2:], np.int64).reshape(v[1], 2))
            ops.append(("set", slots, bows))
            i += 1 + int(t[1])
        elif t[0] == "S":
            ops.append(("sync", parse_trace([lines[i + 1]])[0]))
            i += 2
        else:
            assert t[0] == "C", lines[i]
            ops.append(("clear",))
            i += 1
    return ops


def sequence(tmp):
    """Builds the harness (no sanitizer: its report is tests/test_mapdb_tri_cpu.py's business), runs it and returns its operations."""
    import subprocess
    exe, ops = os.path.join(tmp, "mapdb_bow_check"), os.path.join(tmp, "ops.txt")
    subprocess.check_call(["g++", "-std=c++17", "-O1", CHECK_SRC, "-o", exe])
    subprocess.run([exe, ops], stdout=subprocess.DEVNULL, check=True)
    return read_ops(ops)


def scenario_blob(scene, abort_after):
    """The scenario file of tests/cpp_host/localmapping_run.cpp and createpoints_resident_run.cpp for a scene whose rows are empty."""
    assert all((k["row"] < 0).all() for k in scene.kfs)
    v0 = scene.kfs[0]["view"]
    b = [np.array([v0["fx"], v0["fy"], v0["cx"], v0["cy"], v0["b"], v0["bf"]], f32).tobytes(),
         np.array([len(v0["scale_factors"])], np.int32).tobytes(), v0["scale_factors"].tobytes(), v0["level_sigma2"].tobytes(),
         np.array([len(scene.kfs), abort_after], np.int32).tobytes()]
    for k in scene.kfs:
        v, (ids, start, feat) = k["view"], k["fv"]
        b += [np.ascontiguousarray(v["Tcw"][:, :3]).tobytes(), np.ascontiguousarray(v["Tcw"][:, 3]).tobytes(), v["Ow"].tobytes(),
              np.array([len(v["kps"])], np.int32).tobytes(), v["kps"].tobytes(), k["desc"].tobytes(), v["right_x"].tobytes(), v["depth"].tobytes(),
              np.array([len(ids)], np.int32).tobytes()]
        for i, node in enumerate(ids):
            f = feat[start[i]:start[i + 1]].astype(np.uint32)
            b += [np.array([node], np.uint32).tobytes(), np.array([len(f)], np.int32).tobytes(), f.tobytes()]
    return b"".join(b)
