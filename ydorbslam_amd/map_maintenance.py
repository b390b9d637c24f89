"""Map maintenance on the GPU through the C ABI (include/ydorb/c_api.h, "Map maintenance"): the three passes over the flattened
observation table (map point -> observing keyframes) that restate ORB-SLAM2's MapPoint::UpdateNormalAndDepth, the counting loop of
KeyFrame::UpdateConnections and the counting of LocalMapping::KeyFrameCulling.  DESIGN.md sections 2 ("Map maintenance") and 6l list
the arithmetic and the assumptions.  The three calls take `fn`, another function with the entry's C signature to call in place of the
library's: the tests pass their CPU restatement through it, so both sides go through one argument preparation."""
import ctypes as C

import numpy as np

from ._lib import YdObservationTable, check, lib

COVIS_WINDOW = 8192   # keyframe slots one LDS histogram covers: maptable::kCovisWindow of csrc/map_table.h
UPDATED, BAD, NO_OBSERVATIONS = range(3)
STEREO = 0x80         # bit 7 of an observation's level byte


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _csr(lists, dtype):
    lists = [np.asarray(a, dtype).reshape(-1) for a in lists]
    start = np.concatenate([[0], np.cumsum([len(a) for a in lists], dtype=np.int64)])
    assert start[-1] <= np.iinfo(np.int32).max
    return start.astype(np.int32), np.ascontiguousarray(np.concatenate(lists + [np.zeros(0, dtype)]))


class ObservationTable:
    """The YdObservationTable of n_points map points over n_keyframes keyframe slots.  observers[p] = the observing keyframe slots of
    point p in the iteration order of the reference's observation map, levels[p] = the octaves of the observing keypoints, stereo[p] =
    per observation whether its right x is >= 0 (None: all monocular), bad [n_points] = isBad() (None: none).  Keeps the arrays the
    struct points at alive."""

    def __init__(self, n_keyframes, observers, levels, stereo=None, bad=None):
        self.n_points, self.n_keyframes = len(observers), int(n_keyframes)
        self.obs_start, self.obs_kf = _csr(observers, np.int32)
        _, lv = _csr(levels, np.uint8)
        assert len(lv) == len(self.obs_kf) and (lv < 128).all()
        if stereo is not None:
            _, st = _csr(stereo, np.uint8)
            assert len(st) == len(lv)
            lv = lv | np.where(st != 0, STEREO, 0).astype(np.uint8)
        self.obs_level = np.ascontiguousarray(lv, np.uint8)
        self.bad = np.zeros(self.n_points, np.uint8) if bad is None else np.ascontiguousarray(bad, np.uint8).reshape(-1)
        assert len(self.bad) == self.n_points
        self._sync()

    @classmethod
    def from_arrays(cls, n_keyframes, obs_start, obs_kf, obs_level, bad):
        """The table from already flat arrays (obs_level carries the stereo bit)."""
        T = cls.__new__(cls)
        T.obs_start = np.ascontiguousarray(obs_start, np.int32)
        T.obs_kf, T.obs_level = np.ascontiguousarray(obs_kf, np.int32), np.ascontiguousarray(obs_level, np.uint8)
        T.bad = np.ascontiguousarray(bad, np.uint8)
        T.n_points, T.n_keyframes = len(T.obs_start) - 1, int(n_keyframes)
        T._sync()
        return T

    def _sync(self):
        self.struct = YdObservationTable(self.n_points, self.n_keyframes, _p(self.obs_start), _p(self.obs_kf), _p(self.obs_level), _p(self.bad))

    def span_lengths(self):
        return np.diff(self.obs_start.astype(np.int64))


def update_normal_depth(table, pos, centre, ref_kf, ref_level, scale_factors, device=0, fn=None):
    """One ydorb_map_update_normal_depth call.  Returns dict(normal [n, 3], min_distance [n], max_distance [n], status [n])."""
    n = table.n_points
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    centre = np.ascontiguousarray(centre, np.float32).reshape(-1, 3)
    ref_kf, ref_level = np.ascontiguousarray(ref_kf, np.int32).reshape(-1), np.ascontiguousarray(ref_level, np.uint8).reshape(-1)
    sf = np.ascontiguousarray(scale_factors, np.float32).reshape(-1)
    assert len(pos) == len(ref_kf) == len(ref_level) == n and len(centre) == table.n_keyframes
    normal, mn, mx, st = np.zeros((max(n, 1), 3), np.float32), np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.uint8)
    fn = fn or lib().ydorb_map_update_normal_depth
    check(fn(C.byref(table.struct), _p(pos), _p(centre), _p(ref_kf), _p(ref_level), _p(sf), len(sf), device, _p(normal), _p(mn), _p(mx), _p(st)))
    return dict(normal=normal[:n], min_distance=mn[:n], max_distance=mx[:n], status=st[:n])


def capacity_bounds(table, lists):
    """Per query min(n_keyframes - 1, sum of the listed points' span lengths): what always fits (maptable::capacityBound)."""
    span = table.span_lengths()
    return [max(0, min(table.n_keyframes - 1, int(span[np.asarray(a, np.int64).reshape(-1)].sum()))) for a in lists]


def covisibility(table, query_kf, lists, capacities=None, device=0, fn=None):
    """One ydorb_map_covisibility call: lists[q] = the non-null map-point entries of keyframe query_kf[q].  capacities = per query how
    many connections fit (default: the tight bound).  Returns per query dict(kf, weight, count, status); kf / weight are empty when the
    capacity was too small (status 1)."""
    query_kf = np.ascontiguousarray(query_kf, np.int32).reshape(-1)
    Q = len(query_kf)
    assert len(lists) == Q
    list_start, idx = _csr(lists, np.int32)
    caps = capacity_bounds(table, lists) if capacities is None else [int(c) for c in capacities]
    out_start, _ = _csr([np.zeros(c, np.int32) for c in caps], np.int32)
    total = int(out_start[-1])
    kf, w = np.full(max(total, 1), -1, np.int32), np.full(max(total, 1), -1, np.int32)
    counts, status = np.zeros(max(Q, 1), np.int32), np.zeros(max(Q, 1), np.uint8)
    fn = fn or lib().ydorb_map_covisibility
    check(fn(C.byref(table.struct), _p(query_kf), Q, _p(list_start), _p(idx), _p(out_start), device, _p(kf), _p(w), _p(counts), _p(status)))
    out = []
    for q in range(Q):
        m = int(counts[q]) if status[q] == 0 else 0
        out.append(dict(kf=kf[out_start[q]:out_start[q] + m].copy(), weight=w[out_start[q]:out_start[q] + m].copy(), count=int(counts[q]),
                        status=int(status[q]), raw_kf=kf[out_start[q]:out_start[q + 1]].copy(), raw_weight=w[out_start[q]:out_start[q + 1]].copy()))
    return out


def keyframe_redundancy(table, cand_kf, lists, own_levels, removed=None, th_obs=3, device=0, fn=None):
    """One ydorb_map_keyframe_redundancy call: lists[k] / own_levels[k] = candidate cand_kf[k]'s entries that pass the depth test and the
    octaves of its own keypoints.  Returns dict(n_counted [K], n_redundant [K], cull [K])."""
    cand_kf = np.ascontiguousarray(cand_kf, np.int32).reshape(-1)
    K = len(cand_kf)
    assert len(lists) == len(own_levels) == K
    list_start, idx = _csr(lists, np.int32)
    _, own = _csr(own_levels, np.uint8)
    assert len(own) == len(idx)
    if removed is not None:
        removed = np.ascontiguousarray(removed, np.uint8).reshape(-1)
        assert len(removed) == table.n_keyframes
    nc, nr, cull = np.zeros(max(K, 1), np.int32), np.zeros(max(K, 1), np.int32), np.zeros(max(K, 1), np.uint8)
    fn = fn or lib().ydorb_map_keyframe_redundancy
    check(fn(C.byref(table.struct), _p(cand_kf), K, _p(list_start), _p(idx), _p(own), _p(removed), int(th_obs), device, _p(nc), _p(nr), _p(cull)))
    return dict(n_counted=nc[:K], n_redundant=nr[:K], cull=cull[:K])


def release(device=0):
    """ydorb_map_release: give the map-maintenance scratch of `device` back."""
    check(lib().ydorb_map_release(device))
