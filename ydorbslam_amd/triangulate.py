"""LocalMapping::createNewMapPoints' geometry between searchForTriangulation's matches and the new MapPoints, on the GPU through the C
ABI (include/ydorb/c_api.h, "LocalMapping::createNewMapPoints"): parallax, linear triangulation or stereo unprojection, depth,
reprojection and scale-consistency tests, one lane per match.  Restates ORB-SLAM2's LocalMapping::CreateNewMapPoints, which YDORBSLAM
renames; DESIGN.md section 6f lists the assumptions."""
import ctypes as C

import numpy as np

from ._lib import YdTriBatch, YdTriView, check, lib
from .extractor import KP_DTYPE

# low nibble of a status byte
ACCEPTED, NO_METHOD, W_ZERO, DEPTH_FIRST, DEPTH_SECOND, REPROJ_FIRST, REPROJ_SECOND, ZERO_DISTANCE, SCALE_RATIO, BAD_STEREO_DEPTH = range(10)
SRC_LINEAR, SRC_UNPROJECT_FIRST, SRC_UNPROJECT_SECOND = 1, 2, 3
NOT_FINITE = 0x80


def exit_code(status):
    return np.asarray(status) & 15


def source(status):
    return (np.asarray(status) >> 4) & 3


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _dot3f(A, X):
    """Rows of A times X in the project's float cv::Mat contract: products exact in double, summed in ascending k, rounded once."""
    A = np.asarray(A, np.float32).astype(np.float64)
    X = np.asarray(X, np.float32).astype(np.float64)
    return ((A[..., 0] * X[..., 0] + A[..., 1] * X[..., 1]) + A[..., 2] * X[..., 2]).astype(np.float32)


def make_view(kps, right_x, depth, Tcw, K, b, bf, scale_factor=1.2, n_levels=8, level_sigma2=None, scale_factors=None):
    """One keyframe as YdTriView reads it.  kps: KP_DTYPE records or an [n, 3] array of x, y, octave.  Rwc = Rcw^T and Ow = -Rwc tcw
    as KeyFrame::setPose forms them in float; invfx = 1 / fx in float; the level tables default to the extractor's powers."""
    if not (isinstance(kps, np.ndarray) and kps.dtype == KP_DTYPE):
        a = np.asarray(kps, np.float64).reshape(-1, 3)
        kps = np.zeros(len(a), KP_DTYPE)
        kps["x"], kps["y"], kps["octave"], kps["class_id"] = a[:, 0], a[:, 1], a[:, 2].astype(np.int32), -1
    T = np.ascontiguousarray(np.asarray(Tcw, np.float32).reshape(3, 4))
    Rwc = np.ascontiguousarray(T[:, :3].T)
    Ow = -_dot3f(Rwc, T[:, 3][None, :])
    if scale_factors is None:
        scale_factors = np.ones(n_levels, np.float32)
        for i in range(1, n_levels):
            scale_factors[i] = scale_factors[i - 1] * np.float32(scale_factor)
    scale_factors = np.ascontiguousarray(scale_factors, np.float32)
    if level_sigma2 is None:
        level_sigma2 = scale_factors * scale_factors
    fx, fy, cx, cy = (np.float32(v) for v in K)
    return dict(kps=np.ascontiguousarray(kps), right_x=np.ascontiguousarray(right_x, np.float32), depth=np.ascontiguousarray(depth, np.float32),
                Tcw=T, Rwc=Rwc, Ow=Ow.astype(np.float32), fx=fx, fy=fy, cx=cx, cy=cy, invfx=np.float32(1) / fx, invfy=np.float32(1) / fy,
                b=np.float32(b), bf=np.float32(bf), level_sigma2=np.ascontiguousarray(level_sigma2, np.float32), scale_factors=scale_factors)


class TriBatch:
    """The YdTriBatch of a list of views (make_view dicts) and problems (dicts with first, second: view indices; idx1, idx2 [m]; and
    optionally ratio_factor, default 1.5f * the first view's scale_factors[1]).  Keeps the arrays the struct points at alive."""

    def __init__(self, views, problems, device=0):
        self.views, self.n = views, len(problems)
        self._v = (YdTriView * max(len(views), 1))()
        for i, d in enumerate(views):
            V = self._v[i]
            V.kps, V.right_x, V.depth, V.n = _p(d["kps"]), _p(d["right_x"]), _p(d["depth"]), len(d["kps"])
            V.Tcw[:] = [float(x) for x in np.asarray(d["Tcw"], np.float32).reshape(-1)]
            V.Rwc[:] = [float(x) for x in np.asarray(d["Rwc"], np.float32).reshape(-1)]
            V.Ow[:] = [float(x) for x in np.asarray(d["Ow"], np.float32).reshape(-1)]
            for k in ("fx", "fy", "cx", "cy", "invfx", "invfy", "b", "bf"):
                setattr(V, k, float(d[k]))
            V.level_sigma2, V.scale_factors, V.n_levels = _p(d["level_sigma2"]), _p(d["scale_factors"]), len(d["scale_factors"])
        i32 = lambda k: [np.asarray(p[k], np.int32).reshape(-1) for p in problems]
        i1, i2 = i32("idx1"), i32("idx2")
        self.start = np.concatenate([[0], np.cumsum([len(a) for a in i1])]).astype(np.int32)
        self.idx1 = np.ascontiguousarray(np.concatenate(i1 + [np.zeros(0, np.int32)]))
        self.idx2 = np.ascontiguousarray(np.concatenate(i2 + [np.zeros(0, np.int32)]))
        self.first = np.array([p["first"] for p in problems], np.int32)
        self.second = np.array([p["second"] for p in problems], np.int32)
        rf = []
        for p in problems:
            if "ratio_factor" in p:
                rf.append(np.float32(p["ratio_factor"]))
            else:
                sf = views[p["first"]]["scale_factors"] if 0 <= p["first"] < len(views) else np.ones(2, np.float32)
                rf.append(np.float32(1.5) * np.float32(sf[1] if len(sf) > 1 else 1))
        self.ratio = np.array(rf, np.float32)
        self.M = int(self.start[-1])
        self.struct = YdTriBatch(device, len(views), self.n, C.cast(self._v, C.c_void_p), _p(self.first), _p(self.second), _p(self.start),
                                 _p(self.idx1), _p(self.idx2), _p(self.ratio))

    def outputs(self):
        return np.zeros((max(self.M, 1), 3), np.float32), np.zeros(max(self.M, 1), np.uint8), np.zeros(max(self.n, 1), np.int32)

    def split(self, x3d, status, nacc):
        s = self.start
        return [dict(x3d=x3d[s[p]:s[p + 1]].copy(), status=status[s[p]:s[p + 1]].copy(), n_accepted=int(nacc[p])) for p in range(self.n)]


def triangulate_matches(views, problems, device=0):
    """One ydorb_triangulate_matches call.  Returns per problem dict(x3d [m, 3] float32, status [m] uint8, n_accepted)."""
    B = TriBatch(views, problems, device)
    x3d, status, nacc = B.outputs()
    check(lib().ydorb_triangulate_matches(C.byref(B.struct), _p(x3d), _p(status), _p(nacc)))
    return B.split(x3d, status, nacc)


def release(device=0):
    """ydorb_triangulate_release: give the triangulation scratch of `device` back."""
    check(lib().ydorb_triangulate_release(device))
