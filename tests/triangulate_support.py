"""Test support of createNewMapPoints' geometry: builds the CPU restatement tests/triangulate_ref/triangulate_ref.cpp with
oracle/Makefile's compiler flags, hand-built two-view cases and the synthetic keyframe scene of the GPU parity tests."""
import ctypes as C
import os
import re
import shlex
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "triangulate_ref", "triangulate_ref.cpp")
_REF = None

K = (520.0, 515.0, 320.0, 240.0)
B = 0.12                      # stereo baseline, metres
BF = float(np.float32(B) * np.float32(K[0]))


def _flags():
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return shlex.split(re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1))


def ref():
    global _REF
    if _REF is None:
        out = os.path.join(tempfile.mkdtemp(prefix="triref"), "libtriref.so")
        subprocess.check_call(["g++", *_flags(), "-shared", "-o", out, SRC, "-lm"])
        L = C.CDLL(out)
        L.triref_triangulate.restype = C.c_int
        L.triref_triangulate.argtypes = [C.c_void_p] * 4
        L.triref_null_vector.restype = C.c_int
        L.triref_null_vector.argtypes = [C.c_void_p, C.c_void_p]
        L.triref_cos_stereo.restype = C.c_float
        L.triref_cos_stereo.argtypes = [C.c_float, C.c_float]
        _REF = L
    return _REF


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def ref_triangulate(views, problems):
    """The restatement on the views / problems of ydorbslam_amd.triangulate.triangulate_matches; same return value."""
    from ydorbslam_amd.triangulate import TriBatch
    Bt = TriBatch(views, problems)
    x3d, status, nacc = Bt.outputs()
    ref().triref_triangulate(C.byref(Bt.struct), _p(x3d), _p(status), _p(nacc))
    return Bt.split(x3d, status, nacc)


def ref_null_vector(A):
    A = np.ascontiguousarray(A, np.float32).reshape(4, 4)
    x = np.zeros(4, np.float32)
    sweeps = ref().triref_null_vector(_p(A), _p(x))
    return x, sweeps


def ref_cos_stereo(b, d):
    return np.float32(ref().triref_cos_stereo(C.c_float(b), C.c_float(d)))


# ------------------------------------------------------------------------------------------------------------ geometry helpers
def rot(axis, angle):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    S = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * S + (1 - np.cos(angle)) * S @ S


def pose(R=np.eye(3), centre=(0, 0, 0)):
    """Tcw 3x4 (double) of a camera with rotation Rcw = R and centre `centre` in the world."""
    R = np.asarray(R, np.float64)
    return np.hstack([R, (-R @ np.asarray(centre, np.float64))[:, None]])


def project(T, X):
    """Pixel (u, v) and depth z of world points X [n, 3] in the camera Tcw = T, in double."""
    Xc = np.asarray(X, np.float64) @ T[:, :3].T + T[:, 3]
    return np.stack([K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]], axis=1), Xc[:, 2]


class ViewBuilder:
    """Collects the features of one keyframe; view() gives the make_view dict."""

    def __init__(self, T):
        self.T = np.asarray(T, np.float64)
        self.rows = []      # x, y, octave, right_x, depth
        self.stale_Rwc = None
        self.stale_Ow = None

    def add(self, uv, octave=0, stereo_depth=None, right_noise=0.0):
        """One feature; stereo_depth = its depth z when it carries a stereo measurement.  Returns its index."""
        if stereo_depth is None:
            self.rows.append((uv[0], uv[1], octave, -1.0, -1.0))
        else:
            self.rows.append((uv[0], uv[1], octave, uv[0] - BF / stereo_depth + right_noise, stereo_depth))
        return len(self.rows) - 1

    def add_raw(self, x, y, octave, right_x, depth):
        self.rows.append((x, y, octave, right_x, depth))
        return len(self.rows) - 1

    def view(self):
        from ydorbslam_amd.triangulate import make_view
        a = np.array(self.rows, np.float64).reshape(-1, 5)
        v = make_view(a[:, :3], a[:, 3], a[:, 4], self.T, K, B, BF)
        if self.stale_Rwc is not None:
            v["Rwc"] = np.ascontiguousarray(self.stale_Rwc, np.float32)
        if self.stale_Ow is not None:
            v["Ow"] = np.ascontiguousarray(self.stale_Ow, np.float32)
        return v


# ------------------------------------------------------------------------------------------------------------ hand-built cases
def hand_cases():
    """name -> (views, problem, expected status byte).  Two cameras looking down +z; the second 0.5 m (or 5 cm) to the right.  Every
    case is one match.  Cases 2 and 7 and the NaN case need a view whose Rwc / Ow do not belong to its Tcw (the ABI takes them
    separately, and in the reference they are separate getters that a pose update can fall between): with consistent views w == 0
    needs parallel rays, which the parallax test sends elsewhere, and a point at a camera centre has z = 0 and leaves at the depth
    test."""
    X = np.array([[0.2, 0.1, 4.0]])
    wide, narrow = pose(centre=(0.5, 0, 0)), pose(centre=(0.05, 0, 0))
    cases = {}

    def two(T2, uv1, uv2, o1=0, o2=0, d1=None, d2=None, raw1=None, raw2=None, stale=None):
        a, b = ViewBuilder(pose()), ViewBuilder(T2)
        a.add_raw(*raw1) if raw1 else a.add(uv1, o1, d1)
        b.add_raw(*raw2) if raw2 else b.add(uv2, o2, d2)
        if stale:
            stale(a, b)
        return [a.view(), b.view()], dict(first=0, second=1, idx1=[0], idx2=[0])

    (u1, z1), (u2, z2) = project(pose(), X), project(wide, X)
    (n2, zn2) = project(narrow, X)
    cases["accepted_linear"] = two(wide, u1[0], u2[0]) + (0x10,)
    cases["accepted_unproject_first"] = two(narrow, u1[0], n2[0], d1=z1[0]) + (0x20,)
    cases["accepted_unproject_second"] = two(narrow, u1[0], n2[0], d2=zn2[0]) + (0x30,)
    far = np.array([[30.0, 10.0, 1000.0]])
    cases["no_method_low_parallax"] = two(wide, project(pose(), far)[0][0], project(wide, far)[0][0]) + (0x01,)

    def stale_rotation(a, b):   # the second view's Rwc is 1.5 degrees off its Tcw: the rays differ although A says parallel
        b.stale_Rwc = rot((0, 1, 0), np.radians(1.5)).T
    cases["w_zero"] = two(wide, (K[2], K[3]), (K[2], K[3]), stale=stale_rotation) + (0x12,)
    behind = np.array([[0.2, 0.1, -4.0]])
    cases["behind_first"] = two(wide, project(pose(), behind)[0][0], project(wide, behind)[0][0]) + (0x13,)
    ahead = pose(centre=(0, 0, 6.0))
    side = np.array([[1.5, 0.0, 4.0]])
    cases["behind_second"] = two(ahead, project(pose(), side)[0][0], project(ahead, side)[0][0]) + (0x14,)
    cases["reprojection_first"] = two(wide, u1[0] + (0, 20.0), u2[0]) + (0x15,)
    cases["reprojection_second"] = two(wide, u1[0] + (0, 12.0), u2[0], o1=7, o2=0) + (0x16,)
    cases["scale_ratio"] = two(wide, u1[0], u2[0], o1=0, o2=5) + (0x18,)
    cases["bad_stereo_depth"] = two(wide, None, u2[0], raw1=(u1[0][0], u1[0][1], 0, u1[0][0] - 10.0, 0.0)) + (0x29,)

    # zero distance: the first view's Ow is the triangulated point itself, bit for bit (taken from a first pass)
    views, prob, _ = cases["accepted_linear"]
    pt = ref_triangulate(views, [prob])[0]["x3d"][0]

    def stale_centre(a, b):
        a.stale_Ow = pt
    cases["zero_distance"] = two(wide, u1[0], u2[0], stale=stale_centre) + (0x17,)

    def nan_centre(a, b):
        a.stale_Ow = np.array([np.nan, 0, 0], np.float32)
    cases["nan_point_accepted"] = two(narrow, u1[0], n2[0], d1=z1[0], stale=nan_centre) + (0xA0,)
    return cases


# ------------------------------------------------------------------------------------------------------------ synthetic scene
def scene(seed=7, counts=(203, 0, 197, 211), noise=0.7):
    """Three keyframes shared by four problems, (0,1) (1,2) (0,2) (2,1) with `counts` matches: keyframe 0 at the world origin,
    keyframe 1 a 0.45 m sideways neighbour turned a few degrees, keyframe 2 five centimetres from keyframe 0 (less than the stereo
    baseline).  Mixed mono / stereo features, pixel noise, 20 % wrong matches, points behind a camera, far points, octave mismatches.
    Keyframe 2 answers its getters from two pose versions: Rwc is 1.5 degrees off Tcw, and Ow is a point the pair (0,2) triangulates
    (set from a first pass of the restatement), so that w == 0 and a zero distance occur (see hand_cases for why they need that).
    Returns (views, problems)."""
    rng = np.random.default_rng(seed)
    T = [pose(), pose(rot((0.1, 1, 0.05), np.radians(4.0)), (0.45, 0.03, 0.05)), pose(centre=(0.05, 0, 0))]
    vb = [ViewBuilder(t) for t in T]
    vb[2].stale_Rwc = rot((0, 1, 0), np.radians(1.5)).T
    pairs = [(0, 1), (1, 2), (0, 2), (2, 1)]
    problems = []
    for (a, b), n in zip(pairs, counts):
        X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.2, 1.2, n), rng.uniform(1.0, 12.0, n)], axis=1)
        kind = rng.uniform(size=n)
        X[kind < 0.06, 2] = rng.uniform(300, 900, int((kind < 0.06).sum()))            # far: no parallax
        X[(kind >= 0.06) & (kind < 0.10), 2] *= -1                                      # behind both cameras
        near = (kind >= 0.10) & (kind < 0.14)                                           # in front of keyframe 0 / 2, behind keyframe 1
        X[near] = np.stack([rng.uniform(-0.004, 0.004, near.sum()), rng.uniform(-0.004, 0.004, near.sum()),
                            rng.uniform(0.01, 0.04, near.sum())], axis=1)
        i1, i2 = [], []
        for k in range(n):
            o = int(rng.integers(0, 8))
            o2 = o if rng.uniform() > 0.15 else int((o + rng.integers(3, 6)) % 8)        # octave mismatch
            f = []
            for v, oc in ((a, o), (b, o2)):
                uv, z = project(T[v], X[k:k + 1])
                uv = uv[0] + rng.normal(0, noise, 2)
                stereo = rng.uniform() < 0.5 and 0 < z[0] < 40
                f.append(vb[v].add(uv, oc, z[0] if stereo else None, rng.normal(0, noise)))
            i1.append(f[0]); i2.append(f[1])
        i2 = np.array(i2, np.int32)
        wrong = np.nonzero(rng.uniform(size=n) < 0.2)[0]
        if len(wrong) > 1:
            i2[wrong] = i2[np.roll(wrong, 1)]                                           # wrong matches: another point's feature
        if (a, b) == (0, 2):   # both features at the principal point: parallel rays for A, 1.5 degrees apart for the parallax test
            i1.append(vb[0].add((K[2], K[3]))); i2 = np.append(i2, vb[2].add((K[2], K[3])))
        problems.append(dict(first=a, second=b, idx1=np.array(i1, np.int32), idx2=i2.astype(np.int32)))
    views = [v.view() for v in vb]
    r = ref_triangulate(views, problems)[2]
    ok = np.nonzero(r["status"] == 0x10)[0]
    vb[2].stale_Ow = r["x3d"][ok[0]]
    return [v.view() for v in vb], problems


def explicit_rows():
    """One batch of the hand-built cases the scene cannot give: exit 9 and the accepted non-finite point (and the rest for good measure).
    Returns (views, problems, expected status per problem)."""
    views, problems, want = [], [], []
    for name, (v, p, st) in hand_cases().items():
        problems.append(dict(p, first=len(views), second=len(views) + 1))
        views += v
        want.append(st)
    return views, problems, want
