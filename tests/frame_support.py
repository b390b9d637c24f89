"""Test support of the Frame constructor's tail: builds the CPU restatement tests/frame_ref/frame_ref.cpp with oracle/Makefile's compiler
flags, and holds the three cameras, the seeded point sets, the batch scene and the comparisons the CPU and GPU tests share."""
import ctypes as C
import os
import re
import shlex
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "frame_ref", "frame_ref.cpp")
_REF = None
f32 = np.float32

TUM_K = (517.306408, 516.469215, 318.643040, 255.313989)
# name -> (K, dist = k1 k2 p1 p2 k3, (w, h))
CAMERAS = {
    "tum_fr1": (TUM_K, (0.262383, -0.953104, -0.005358, 0.002628, 1.163314), (640, 480)),
    "barrel": ((458.654, 457.296, 367.215, 248.375), (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0), (752, 480)),
    "pinhole": (TUM_K, (0.0, 0.0, 0.01, 0.0, 0.0), (640, 480)),
}
BF = 40.0


def _flags():
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return shlex.split(re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1))


def ref():
    global _REF
    if _REF is None:
        out = os.path.join(tempfile.mkdtemp(prefix="frameref"), "libframeref.so")
        subprocess.check_call(["g++", *_flags(), "-shared", "-o", out, SRC, "-lm"])
        L = C.CDLL(out)
        L.frameref_undistort_points.restype = None
        L.frameref_undistort_points.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.frameref_image_bounds.restype = None
        L.frameref_image_bounds.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.frameref_frame_tail.restype = None
        L.frameref_frame_tail.argtypes = [C.c_void_p] * 7
        _REF = L
    return _REF


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def cam(name, n_iter=5):
    from ydorbslam_amd.frame import camera
    K, dist, _ = CAMERAS[name]
    return camera(K, dist, n_iter)


def size(name):
    return CAMERAS[name][2]


def points(name, n=2000, seed=11):
    """n seeded points over the camera's image, [n, 2] float32."""
    w, h = size(name)
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n)], axis=1).astype(f32)


def keypoints(xy, seed=3):
    from ydorbslam_amd import KP_DTYPE
    rng = np.random.default_rng(seed)
    k = np.zeros(len(xy), KP_DTYPE)
    k["x"], k["y"] = xy[:, 0], xy[:, 1]
    k["size"], k["angle"], k["response"] = 31.0, rng.uniform(0, 360, len(xy)), rng.uniform(1, 200, len(xy))
    k["octave"], k["class_id"] = rng.integers(0, 8, len(xy)), -1
    return k


# ------------------------------------------------------------------------------------------------------------ the restatement
def ref_undistort(camera, xy):
    """(undistorted [n, 2] float32, status word)."""
    xy = np.ascontiguousarray(xy, f32).reshape(-1, 2)
    out = np.zeros_like(xy)
    st = C.c_int(0)
    ref().frameref_undistort_points(C.byref(camera), _p(xy), len(xy), _p(out), C.byref(st))
    return out, st.value


def ref_bounds(camera, w, h):
    b = np.zeros(4, f32)
    ref().frameref_image_bounds(C.byref(camera), w, h, _p(b))
    return b


def ref_tail(camera, kps, n, depth=None, samples=False, factor=1.0, bf=0.0, bounds=None, flags=0):
    """The restatement on the arguments of ydorbslam_amd.frame.frame_tail; the same dict with every output."""
    from ydorbslam_amd import KP_DTYPE
    from ydorbslam_amd._lib import YdFrameTail
    from ydorbslam_amd.frame import GRID_CELLS, _depth_type
    kps = np.ascontiguousarray(kps, KP_DTYPE)
    F, cap = kps.shape
    n = np.ascontiguousarray(n, np.int32).reshape(F)
    T = YdFrameTail()
    T.kps, T.n, T.n_frames, T.cap = _p(kps), _p(n), F, cap
    T.depth_type = _depth_type(depth, samples)
    if depth is not None:
        if samples:
            depth = np.ascontiguousarray(depth, f32).reshape(F, cap)
        else:
            T.depth_h, T.depth_w = depth.shape[1], depth.shape[2]
            T.depth_frame_stride, T.depth_row_stride = depth.strides[0], depth.strides[1]
        T.depth = depth.ctypes.data
    T.depth_factor, T.bf, T.cam, T.flags = float(factor), float(bf), camera, int(flags)
    grid = bounds is not None
    if grid:
        T.bounds[:] = [float(b) for b in bounds]
    o = dict(kps_un=np.zeros((F, cap), KP_DTYPE), right_x=np.zeros((F, cap), f32), depth=np.zeros((F, cap), f32),
             cell_start=np.zeros((F, GRID_CELLS + 1), np.int32) if grid else None, cell_idx=np.zeros((F, cap), np.int32) if grid else None,
             status=np.zeros(F, np.int32))
    ref().frameref_frame_tail(C.byref(T), _p(o["kps_un"]), _p(o["right_x"]), _p(o["depth"]), _p(o["cell_start"]), _p(o["cell_idx"]), _p(o["status"]))
    return o


# ------------------------------------------------------------------------------------------------------------ independent statements
def numpy_undistort(name, xy, n_iter=5):
    """The contract's loop in numpy float64, vectorised over the points (its own code: nothing shared with the restatement)."""
    K, dist, _ = CAMERAS[name]
    fx, fy, cx, cy = (np.float64(f32(k)) for k in K)
    k1, k2, p1, p2, k3 = (np.float64(f32(d)) for d in dist)
    xy = np.asarray(xy, f32)
    if f32(dist[0]) == 0:
        return xy.copy(), np.zeros(len(xy), bool)
    ifx, ify = np.float64(1.0) / fx, np.float64(1.0) / fy
    x0 = (xy[:, 0].astype(np.float64) - cx) * ifx
    y0 = (xy[:, 1].astype(np.float64) - cy) * ify
    x, y = x0.copy(), y0.copy()
    live = np.ones(len(xy), bool)      # points whose loop still runs
    for _ in range(n_iter):
        r2 = x * x + y * y
        with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
            icdist = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
            neg = live & (icdist < 0)
            dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
            dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
            nx, ny = (x0 - dx) * icdist, (y0 - dy) * icdist
        x = np.where(neg, x0, np.where(live, nx, x))
        y = np.where(neg, y0, np.where(live, ny, y))
        live &= ~neg
    return np.stack([(fx * x + cx).astype(f32), (fy * y + cy).astype(f32)], axis=1), ~live


def distort(name, xy):
    """The forward model in float64: where the undistorted pixel xy is seen in the distorted image."""
    K, dist, _ = CAMERAS[name]
    fx, fy, cx, cy = K
    k1, k2, p1, p2, k3 = dist
    x, y = (np.asarray(xy[:, 0], np.float64) - cx) / fx, (np.asarray(xy[:, 1], np.float64) - cy) / fy
    r2 = x * x + y * y
    cd = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = x * cd + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * cd + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return np.stack([fx * xd + cx, fy * yd + cy], axis=1)


def csr_lists(cell_start, cell_idx):
    """The CSR of one frame as {cell: [indices]} over the non-empty cells."""
    return {c: cell_idx[cell_start[c]:cell_start[c + 1]].tolist() for c in np.nonzero(np.diff(cell_start))[0]}


# ------------------------------------------------------------------------------------------------------------ comparisons
def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_keypoints(got, want):
    from ydorbslam_amd import KP_DTYPE
    assert got.shape == want.shape
    assert np.array_equal(np.ascontiguousarray(got, KP_DTYPE).view(np.uint32), np.ascontiguousarray(want, KP_DTYPE).view(np.uint32))


def same_tail(got, want, n, grid=True):
    """Every output of frame_tail that `got` holds, bit for bit over the first n[f] slots of frame f."""
    for f in range(len(n)):
        k = int(n[f])
        if got["kps_un"] is not None:
            same_keypoints(got["kps_un"][f, :k], want["kps_un"][f, :k])
        for key in ("right_x", "depth"):
            if got[key] is not None:
                assert np.array_equal(bits(got[key][f, :k]), bits(want[key][f, :k])), (key, f)
        if grid and got["cell_start"] is not None:
            assert np.array_equal(got["cell_start"][f], want["cell_start"][f]), f
            m = int(want["cell_start"][f, -1])
            assert np.array_equal(got["cell_idx"][f, :m], want["cell_idx"][f, :m]), f
    if got["status"] is not None:
        assert np.array_equal(got["status"], want["status"])


# ------------------------------------------------------------------------------------------------------------ the batch scene
CAP = 512
COUNTS = (300, 0, CAP)


def batch(name, seed=21):
    """Three frames of one camera with counts 300, 0 and cap = 512: keypoints [3, 512] over the whole image (a few on the last row and
    column), slots past the count filled with a far-away sentinel that must never be read."""
    w, h = size(name)
    rng = np.random.default_rng(seed)
    xy = np.stack([rng.uniform(0, w, 3 * CAP), rng.uniform(0, h, 3 * CAP)], axis=1).astype(f32)
    xy[::97, 0] = f32(w) - f32(0.01)
    xy[::89, 1] = f32(h) - f32(0.01)
    kps = keypoints(xy, seed).reshape(3, CAP)
    n = np.array(COUNTS, np.int32)
    for f in range(3):
        kps["x"][f, n[f]:] = 1e9
        kps["y"][f, n[f]:] = -1e9
    return kps, n


def depth_images(shape, seed=31):
    """(uint16 [3, h, w], float32 [3, h, w]) for shape = (w, h): a fifth of the pixels without depth (0), a few negative or NaN in the float
    image, and 65535 in the uint16 one."""
    w, h = shape
    rng = np.random.default_rng(seed)
    u16 = rng.integers(300, 40000, (3, h, w)).astype(np.uint16)
    u16[rng.uniform(size=u16.shape) < 0.2] = 0
    u16[rng.uniform(size=u16.shape) < 0.01] = 65535
    flt = rng.uniform(0.3, 9.0, (3, h, w)).astype(f32)
    r = rng.uniform(size=flt.shape)
    flt[r < 0.2] = 0.0
    flt[(r >= 0.2) & (r < 0.22)] = -1.5
    flt[(r >= 0.22) & (r < 0.24)] = np.nan
    return u16, flt


def padded(img, extra=24):
    """A view of img [F, h, w] inside an array whose rows are `extra` elements longer: a row stride larger than the row."""
    F, h, w = img.shape
    big = np.full((F, h, w + extra), 77, img.dtype)
    big[:, :, :w] = img
    return big[:, :, :w]
