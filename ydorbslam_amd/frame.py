"""The RGB-D Frame constructor's tail on the GPU through the C ABI (include/ydorb/c_api.h, "Frame construction"): undistortKeyPoints,
computeStereoFromRGBD, computeImageBounds and assignKeyPointsToGrid (reference src/frame.cpp:99-100,134-145), for batches of frames,
and the per-frame single call behind extractAndCompute.  Restates ORB-SLAM2's Frame::UndistortKeyPoints / ComputeStereoFromRGBD /
ComputeImageBounds / AssignFeaturesToGrid, which YDORBSLAM renames; DESIGN.md sections 2 ("Frame tail") and 6h list the assumptions."""
import ctypes as C

import numpy as np

from ._lib import YdCamera, YdFrameTail, check, lib
from .extractor import KP_DTYPE

DEPTH_NONE, DEPTH_U16, DEPTH_F32, DEPTH_SAMPLES = range(4)
DEPTH_AT_UNDISTORTED, DEVICE_POINTERS = 1, 2
STATUS_DEPTH_INDEX, STATUS_ICDIST = 1, 4
GRID_CELLS = 64 * 48


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def camera(K, dist=(0, 0, 0, 0, 0), n_iter=5):
    """YdCamera of K = (fx, fy, cx, cy) and dist = (k1, k2, p1, p2, k3)."""
    cam = YdCamera()
    cam.fx, cam.fy, cam.cx, cam.cy = (float(np.float32(k)) for k in K)
    cam.dist[:] = [float(np.float32(d)) for d in dist]
    cam.n_iter = int(n_iter)
    return cam


def undistort_points(cam, xy, device=0):
    """ydorb_undistort_points: xy [n, 2] float32 -> the undistorted points [n, 2]."""
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    out = np.zeros_like(xy)
    check(lib().ydorb_undistort_points(C.byref(cam), _p(xy), len(xy), _p(out), device))
    return out


def image_bounds(cam, w, h, device=0):
    """ydorb_image_bounds: (min_x, max_x, min_y, max_y) float32 [4]."""
    b = np.zeros(4, np.float32)
    check(lib().ydorb_image_bounds(C.byref(cam), int(w), int(h), _p(b), device))
    return b


def _depth_type(depth, samples):
    if depth is None:
        return DEPTH_NONE
    if samples:
        return DEPTH_SAMPLES
    if depth.dtype == np.uint16:
        return DEPTH_U16
    if depth.dtype == np.float32:
        return DEPTH_F32
    raise TypeError("a depth image is uint16 or float32")


def frame_tail(cam, kps, n, depth=None, samples=False, factor=1.0, bf=0.0, bounds=None, flags=0, want=("kps_un", "right_x", "depth", "grid", "status"),
               device=0):
    """One host-form ydorb_frame_tail call.  kps [F, cap] KP_DTYPE, n [F]; depth: None, [F, h, w] uint16 / float32 (a view with a larger
    row stride is passed as it is) or, with samples=True, [F, cap] float32.  `want` names the outputs; returns dict(kps_un, right_x,
    depth [F, cap], cell_start [F, 3073], cell_idx [F, cap], status [F]) with the ones not asked for None."""
    kps = np.ascontiguousarray(kps, KP_DTYPE)
    F, cap = kps.shape
    n = np.ascontiguousarray(n, np.int32).reshape(F)
    T = YdFrameTail()
    T.kps, T.n, T.n_frames, T.cap = _p(kps), _p(n), F, cap
    T.depth_type = _depth_type(depth, samples)
    if depth is not None:
        if samples:
            depth = np.ascontiguousarray(depth, np.float32).reshape(F, cap)
        else:
            assert depth.ndim == 3 and depth.shape[0] == F and depth.strides[2] == depth.itemsize
            T.depth_h, T.depth_w = depth.shape[1], depth.shape[2]
            T.depth_frame_stride, T.depth_row_stride = depth.strides[0], depth.strides[1]
        T.depth = depth.ctypes.data
    T.depth_factor, T.bf, T.cam, T.flags, T.device = float(factor), float(bf), cam, int(flags) & ~DEVICE_POINTERS, device
    if bounds is not None:
        T.bounds[:] = [float(b) for b in bounds]
    o = dict(kps_un=np.zeros((F, cap), KP_DTYPE) if "kps_un" in want else None,
             right_x=np.zeros((F, cap), np.float32) if "right_x" in want else None,
             depth=np.zeros((F, cap), np.float32) if "depth" in want else None,
             cell_start=np.zeros((F, GRID_CELLS + 1), np.int32) if "grid" in want else None,
             cell_idx=np.zeros((F, cap), np.int32) if "grid" in want else None,
             status=np.zeros(F, np.int32) if "status" in want else None)
    check(lib().ydorb_frame_tail(C.byref(T), _p(o["kps_un"]), _p(o["right_x"]), _p(o["depth"]), _p(o["cell_start"]), _p(o["cell_idx"]),
                                 _p(o["status"]), None))
    return o


def frame_tail_device(cam, d_kps, d_n, n_frames, cap, d_kps_un=None, d_right_x=None, d_depth_out=None, d_cell_start=None, d_cell_idx=None,
                      d_status=None, d_depth=None, depth_type=DEPTH_NONE, depth_w=0, depth_h=0, depth_row_stride=0, depth_frame_stride=0,
                      factor=1.0, bf=0.0, bounds=None, flags=0, stream=None, device=0):
    """The device-pointer form: every d_* is a raw HBM address (e.g. a torch tensor's data_ptr()); asynchronous on `stream`."""
    T = YdFrameTail()
    T.kps, T.n, T.n_frames, T.cap = d_kps, d_n, n_frames, cap
    T.depth, T.depth_type, T.depth_w, T.depth_h = d_depth, depth_type, depth_w, depth_h
    T.depth_row_stride, T.depth_frame_stride = depth_row_stride, depth_frame_stride
    T.depth_factor, T.bf, T.cam, T.flags, T.device = float(factor), float(bf), cam, int(flags) | DEVICE_POINTERS, device
    if bounds is not None:
        T.bounds[:] = [float(b) for b in bounds]
    check(lib().ydorb_frame_tail(C.byref(T), d_kps_un, d_right_x, d_depth_out, d_cell_start, d_cell_idx, d_status, stream))


def extract_rgbd(extractor, gray, depth, cam, bf, bounds, factor=1.0, flags=0, grid=True):
    """ydorb_extract_rgbd on an OrbExtractor: gray [h, w] uint8, depth None or [h, w] uint16 / float32.  Returns dict(kps_raw, kps_un,
    desc, right_x, depth, cell_start, cell_idx, status), the per-keypoint arrays cut to the keypoint count."""
    if gray.dtype != np.uint8 or gray.ndim != 2 or gray.strides[1] != 1:
        raise TypeError("extract_rgbd expects a 2-D uint8 image")
    h, w = gray.shape
    if depth is not None:
        assert depth.shape == (h, w) and depth.strides[1] == depth.itemsize
    cap = extractor.max_keypoints
    kps_raw, kps_un = np.zeros(cap, KP_DTYPE), np.zeros(cap, KP_DTYPE)
    desc = np.zeros((cap, 32), np.uint8)
    right_x, depth_out = np.zeros(cap, np.float32), np.zeros(cap, np.float32)
    cell_start = np.zeros(GRID_CELLS + 1, np.int32) if grid else None
    cell_idx = np.zeros(cap, np.int32) if grid else None
    b = None if bounds is None else np.ascontiguousarray(bounds, np.float32)
    n, status = C.c_int32(0), C.c_int32(0)
    check(lib().ydorb_extract_rgbd(extractor._h, gray.ctypes.data, w, h, gray.strides[0], None if depth is None else depth.ctypes.data,
                                   _depth_type(depth, False), 0 if depth is None else depth.strides[0], float(factor), C.byref(cam), float(bf),
                                   _p(b), int(flags), _p(kps_raw), _p(kps_un), _p(desc), _p(right_x), _p(depth_out), _p(cell_start),
                                   _p(cell_idx), cap, C.byref(n), C.byref(status)))
    k = n.value
    return dict(kps_raw=kps_raw[:k], kps_un=kps_un[:k], desc=desc[:k], right_x=right_x[:k], depth=depth_out[:k], cell_start=cell_start,
                cell_idx=None if cell_idx is None else cell_idx[:k], status=status.value)


def release(device=0):
    """ydorb_frame_release: give the frame-construction scratch of `device` back."""
    check(lib().ydorb_frame_release(device))
