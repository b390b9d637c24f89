"""Tracking::searchLocalPoints' numeric part on the GPU through the C ABI (include/ydorb/c_api.h, "Local map tracking"):
Frame::isInCameraFrustum with MapPoint::predictScaleLevel for batches of (view, map-point list), one lane per entry, and the one-view
form fused with searchByProjectionInFrameAndMapPoint.  Restates ORB-SLAM2's Frame::isInFrustum / MapPoint::PredictScale, which
YDORBSLAM renames; DESIGN.md sections 2 ("isInCameraFrustum") and 6g list the assumptions."""
import ctypes as C

import numpy as np

from ._lib import YdFrustumBatch, YdFrustumView, YdMapPointTable, check, lib

IN_VIEW, SKIPPED, BEHIND, OUT_U, OUT_V, DISTANCE, VIEW_ANGLE = range(7)
TRACK_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("view_cos", "<f4"), ("level", "<i4")])
assert TRACK_DTYPE.itemsize == 20


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def make_view(Tcw, Ow, K, bf, bounds, level_ratio, scale_factors, viewing_cos_limit=0.5):
    """One frame as YdFrustumView reads it.  Tcw 3x4, Ow [3] as the frame holds them, K = (fx, fy, cx, cy), bounds = (min_x, max_x,
    min_y, max_y); level_ratio [n_levels - 1] comes from the host's log (the adapter's levelRatioTable), never from numpy's."""
    T = np.asarray(Tcw, np.float32).reshape(3, 4)
    sf = np.asarray(scale_factors, np.float32).reshape(-1)
    lr = np.asarray(level_ratio, np.float32).reshape(-1)
    V = YdFrustumView()
    V.Rcw[:] = [float(x) for x in T[:, :3].reshape(-1)]
    V.tcw[:] = [float(x) for x in T[:, 3]]
    V.Ow[:] = [float(x) for x in np.asarray(Ow, np.float32).reshape(3)]
    V.fx, V.fy, V.cx, V.cy = (float(np.float32(k)) for k in K)
    V.bf = float(np.float32(bf))
    V.min_x, V.max_x, V.min_y, V.max_y = (float(np.float32(b)) for b in bounds)
    V.viewing_cos_limit = float(np.float32(viewing_cos_limit))
    V.n_levels = len(sf)
    for k in range(min(len(lr), 7)):
        V.level_ratio[k] = float(lr[k])
    for k in range(min(len(sf), 8)):
        V.scale_factors[k] = float(sf[k])
    return V


class PointTable:
    """The YdMapPointTable of n map points: pos, normal [n, 3]; min_dist_inv / max_dist_inv = the invariance getters' values;
    max_distance = the raw m_flt_maxDistance; desc [n, 32] (the searches only).  Keeps the arrays the struct points at alive."""

    def __init__(self, pos, normal, min_dist_inv, max_dist_inv, max_distance, desc=None):
        pos = np.asarray(pos, np.float32).reshape(-1, 3)
        self.n = len(pos)
        self.pos_min = np.ascontiguousarray(np.column_stack([pos, np.asarray(min_dist_inv, np.float32).reshape(-1)]), np.float32)
        self.normal_max = np.ascontiguousarray(np.column_stack([np.asarray(normal, np.float32).reshape(-1, 3),
                                                                np.asarray(max_dist_inv, np.float32).reshape(-1)]), np.float32)
        self.max_distance = np.ascontiguousarray(max_distance, np.float32).reshape(-1)
        self.desc = None if desc is None else np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        assert self.pos_min.shape == self.normal_max.shape == (self.n, 4) and len(self.max_distance) == self.n
        self.struct = YdMapPointTable(_p(self.pos_min), _p(self.normal_max), _p(self.max_distance), _p(self.desc), self.n)


class FrustumBatch:
    """The YdFrustumBatch of views (YdFrustumView), a PointTable and per view a list of point indices with its skip flags."""

    def __init__(self, views, table, lists, skips, device=0):
        self.table, self.F = table, len(views)
        self._v = (YdFrustumView * max(self.F, 1))(*views)
        idx = [np.asarray(a, np.int32).reshape(-1) for a in lists]
        sk = [np.asarray(a, np.uint8).reshape(-1) for a in skips]
        assert len(idx) == len(sk) == self.F and all(len(a) == len(b) for a, b in zip(idx, sk))
        self.start = np.concatenate([[0], np.cumsum([len(a) for a in idx])]).astype(np.int32)
        self.idx = np.ascontiguousarray(np.concatenate(idx + [np.zeros(0, np.int32)]))
        self.skip = np.ascontiguousarray(np.concatenate(sk + [np.zeros(0, np.uint8)]))
        self.L = int(self.start[-1])
        self.struct = YdFrustumBatch(device, self.F, C.cast(self._v, C.c_void_p), table.struct, _p(self.start), _p(self.idx), _p(self.skip))

    def outputs(self):
        return np.zeros(max(self.L, 1), TRACK_DTYPE), np.zeros(max(self.L, 1), np.uint8), np.zeros(max(self.F, 1), np.int32)

    def split(self, rows, status, n_in):
        s = self.start
        return [dict(rows=rows[s[f]:s[f + 1]].copy(), status=status[s[f]:s[f + 1]].copy(), n_in_view=int(n_in[f])) for f in range(self.F)]


def frustum_cull(views, table, lists, skips, device=0):
    """One ydorb_frustum_cull call.  Returns per view dict(rows [m] TRACK_DTYPE, status [m] uint8, n_in_view)."""
    B = FrustumBatch(views, table, lists, skips, device)
    rows, status, n_in = B.outputs()
    check(lib().ydorb_frustum_cull(C.byref(B.struct), _p(rows), _p(status), _p(n_in)))
    return B.split(rows, status, n_in)


def search_local_points(matcher, frame, view, table, skip, has_observations, th, taken=None, assigned=None):
    """One ydorb_search_local_points call on an OrbMatcher handle (its ratio is used).  Returns dict(n_to_match, n_matches, assigned,
    taken, rows, status)."""
    skip = np.ascontiguousarray(skip, np.uint8)
    has_obs = np.ascontiguousarray(has_observations, np.uint8)
    assert len(skip) == len(has_obs) == table.n
    taken = np.zeros(frame.n, np.uint8) if taken is None else np.ascontiguousarray(taken, np.uint8).copy()
    assigned = np.full(frame.n, -1, np.int32) if assigned is None else np.ascontiguousarray(assigned, np.int32).copy()
    rows, status = np.zeros(max(table.n, 1), TRACK_DTYPE), np.zeros(max(table.n, 1), np.uint8)
    n_to, n_m = C.c_int32(0), C.c_int32(0)
    fv = frame.c()
    check(lib().ydorb_search_local_points(matcher._h, C.byref(fv), C.byref(view), C.byref(table.struct), _p(skip), _p(has_obs), float(th),
                                          matcher.ratio, _p(taken), _p(assigned), _p(rows), _p(status), C.byref(n_to), C.byref(n_m)))
    return dict(n_to_match=n_to.value, n_matches=n_m.value, assigned=assigned, taken=taken, rows=rows[:table.n], status=status[:table.n])


def release(device=0):
    """ydorb_frustum_release: give the frustum scratch of `device` back."""
    check(lib().ydorb_frustum_release(device))
