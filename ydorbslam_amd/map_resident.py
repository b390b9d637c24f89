"""The resident map table through the C ABI (include/ydorb/c_api.h, "Resident map table"): the observation table
of map maintenance kept in HBM between calls, changed by deltas and queried with no table upload.  MapDb owns one ydorb_mapdb_t.  Its
three queries go through map_maintenance's own wrappers (same argument preparation, same result dictionaries), with the handle in place
of the flat table.  MapDb.correct (ydorb_mapdb_correct) runs the point loops of loop closing on the table in place.
The keyframe rows add the relation keyframe -> map points and the two set queries of Tracking::updateLocalMap.
The resident descriptors add the keyframes' descriptor blocks and the points' views, and
MapPoint::computeDistinctiveDescriptors over them with no descriptor upload.  The resident point attributes keep
normal, distances and descriptor of every point where those queries compute them, and Tracking::searchLocalPoints reads them by slot.  The resident keyframe features
 add each keyframe's keypoints and right coordinates, and MapDb.fuse_search runs the search of fuseByProjection /
fuseBySim3 for all target keyframes of a LocalMapping::searchInNeighbors direction in one call.  The resident BoW feature vectors
 add each keyframe's DBoW3::FeatureVector, and MapDb.create_new_points runs LocalMapping::createNewMapPoints'
search and geometry for all neighbours in one call.  MapDb.search_by_bow_keyframes / search_by_bow_frame run
OrbMatcher::searchByBowInTwoKeyFrames / searchByBowInKeyFrameAndFrame for all candidate keyframes of a loop or relocalisation round in one call."""
import ctypes as C

import numpy as np

from . import map_maintenance as M
from .extractor import KP_DTYPE
from ._lib import (YdBowSide, YdCreateNeighbour, YdCreateView, YdFuseTarget, YdLocalBaGraph, YdMapCorrection, YdMapDbAttrStats, YdMapDbBowStats,
                   YdMapDbDescStats, YdMapDbFeatStats, YdMapDbLbaStats, YdMapDbRowStats, YdMapDbStats, check, lib)

_p = M._p

ARITHMETIC = {"sim3": 0, "se3": 1}                              # YDORB_MAPCORR_SIM3 / _SE3
CENTRES = {"resident": 0, "interleaved": 1, "poses_first": 2}   # YDORB_MAPCORR_RESIDENT / _INTERLEAVED / _POSES_FIRST
CORRECTION_STATUS = {"done": 0, "bad": 1, "claimed": 2, "not_covered": 3, "done_no_observations": 4}


def correction(kf_slots, before, after, n_all, slots, corrector, arithmetic, centre_after, centres, scale_factors):
    """A YdMapCorrection over numpy arrays.  n_all = the table's n_points when slots is None.  Returns (struct, outputs, the arrays the
    struct points into)."""
    kf_slots = np.ascontiguousarray(kf_slots, np.int32).reshape(-1)
    K = len(kf_slots)
    se3 = ARITHMETIC[arithmetic] == 1
    before = np.ascontiguousarray(before, np.float32 if se3 else np.float64).reshape(K, 12 if se3 else 8)
    after = np.ascontiguousarray(after, np.float32 if se3 else np.float64).reshape(K, 12 if se3 else 8)
    slots = None if slots is None else np.ascontiguousarray(slots, np.int32).reshape(-1)
    n = n_all if slots is None else len(slots)
    corrector = None if corrector is None else np.ascontiguousarray(corrector, np.int32).reshape(-1)
    centre_after = None if centre_after is None else np.ascontiguousarray(centre_after, np.float32).reshape(K, 3)
    sf = None if scale_factors is None else np.ascontiguousarray(scale_factors, np.float32).reshape(-1)
    assert corrector is None or len(corrector) == n
    m = max(n, 1)
    out = dict(pos=np.zeros((m, 3), np.float32), status=np.zeros(m, np.uint8))
    if sf is not None:
        out.update(normal=np.zeros((m, 3), np.float32), min_distance=np.zeros(m, np.float32), max_distance=np.zeros(m, np.float32))
    c = YdMapCorrection(n_kf=K, arithmetic=ARITHMETIC[arithmetic], kf_slots=_p(kf_slots), before=_p(before), after=_p(after),
                        centre_after=_p(centre_after), centres=CENTRES[centres], n=n, slots=_p(slots), corrector=_p(corrector),
                        scale_factors=_p(sf), n_levels=0 if sf is None else len(sf), reserved=0, normal=_p(out.get("normal")),
                        min_distance=_p(out.get("min_distance")), max_distance=_p(out.get("max_distance")), pos_out=_p(out["pos"]),
                        status=_p(out["status"]))
    keep = (kf_slots, before, after, slots, corrector, centre_after, sf, out)
    return c, {k: v[:n] for k, v in out.items()}, keep


class MapDb:
    """One resident table on `device`.  The capacities are initial: every table grows on demand.  Slots are the caller's."""

    def __init__(self, device=0, point_capacity=1024, keyframe_capacity=64, observation_capacity=8192):
        self._h = C.c_void_p()
        check(lib().ydorb_mapdb_create(device, point_capacity, keyframe_capacity, observation_capacity, C.byref(self._h)))
        self._span = np.zeros(0, np.int64)   # span length per point slot, for the covisibility capacity bound

    def close(self):
        if self._h:
            lib().ydorb_mapdb_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:   # interpreter shutdown: the loader may be gone already
            pass

    def clear(self):
        check(lib().ydorb_mapdb_clear(self._h))
        self._span = np.zeros(0, np.int64)

    # ------------------------------------------------------------------------------------------------------------ staging
    def set_centres(self, kf_slots, centre):
        kf_slots = np.ascontiguousarray(kf_slots, np.int32).reshape(-1)
        centre = np.ascontiguousarray(centre, np.float32).reshape(-1, 3)
        assert len(centre) == len(kf_slots)
        check(lib().ydorb_mapdb_set_centres(self._h, _p(kf_slots), len(kf_slots), _p(centre)))

    def set_points(self, slots, observers, levels, bad, ref_kf, ref_level, pos):
        """observers[i] / levels[i] = the observing keyframe slots of point slots[i] in the container's order and their level bytes (bit 7 =
        stereo); bad, ref_kf, ref_level [n]; pos [n, 3]."""
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        n = len(slots)
        start, kf = M._csr(observers, np.int32)
        _, lv = M._csr(levels, np.uint8)
        bad, ref_level = np.ascontiguousarray(bad, np.uint8).reshape(-1), np.ascontiguousarray(ref_level, np.uint8).reshape(-1)
        ref_kf, pos = np.ascontiguousarray(ref_kf, np.int32).reshape(-1), np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        assert len(observers) == len(levels) == len(bad) == len(ref_kf) == len(ref_level) == len(pos) == n and len(kf) == len(lv)
        check(lib().ydorb_mapdb_set_points(self._h, _p(slots), n, _p(start), _p(kf), _p(lv), _p(bad), _p(ref_kf), _p(ref_level), _p(pos)))
        if n:
            if slots.max() >= len(self._span):
                self._span = np.concatenate([self._span, np.zeros(int(slots.max()) + 1 - len(self._span), np.int64)])
            self._span[slots] = np.diff(start.astype(np.int64))   # a repeated slot keeps its last span, as the table does

    def set_positions(self, slots, pos):
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        assert len(pos) == len(slots)
        check(lib().ydorb_mapdb_set_positions(self._h, _p(slots), len(slots), _p(pos)))

    # ------------------------------------------------------------------------------------------------------------ what the wrappers read
    @property
    def n_points(self):
        return self.stats()["n_points"]

    @property
    def n_keyframes(self):
        return self.stats()["n_keyframes"]

    def span_lengths(self):
        return self._span

    # ------------------------------------------------------------------------------------------------------------ queries
    def update_normal_depth(self, slots, scale_factors):
        """ydorb_mapdb_update_normal_depth for the named slots.  Returns dict(normal [n, 3], min_distance, max_distance, status [n])."""
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        sf = np.ascontiguousarray(scale_factors, np.float32).reshape(-1)
        n = len(slots)
        normal, mn, mx, st = np.zeros((max(n, 1), 3), np.float32), np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.uint8)
        check(lib().ydorb_mapdb_update_normal_depth(self._h, _p(slots), n, _p(sf), len(sf), _p(normal), _p(mn), _p(mx), _p(st)))
        return dict(normal=normal[:n], min_distance=mn[:n], max_distance=mx[:n], status=st[:n])

    def covisibility(self, query_kf, lists, capacities=None):
        def fn(_table, q, Q, ls, idx, os_, _device, kf, w, counts, status):
            return lib().ydorb_mapdb_covisibility(self._h, q, Q, ls, idx, os_, kf, w, counts, status)
        return M.covisibility(_Header(self), query_kf, lists, capacities, fn=fn)

    def keyframe_redundancy(self, cand_kf, lists, own_levels, removed=None, th_obs=3):
        def fn(_table, c, K, ls, idx, own, rem, th, _device, nc, nr, cull):
            return lib().ydorb_mapdb_keyframe_redundancy(self._h, c, K, ls, idx, own, rem, th, nc, nr, cull)
        return M.keyframe_redundancy(_Header(self), cand_kf, lists, own_levels, removed, th_obs, fn=fn)

    def correct(self, kf_slots, before, after, slots=None, corrector=None, arithmetic="sim3", centre_after=None, centres="resident",
                scale_factors=None):
        """ydorb_mapdb_correct: the point loops of loop closing in place on the table.  kf_slots [K]; before / after [K, 8] doubles
        (arithmetic "sim3") or [K, 12] floats ("se3"); slots [n] or None = every slot in order; corrector [n] ranks into kf_slots, -1 =
        the point's reference keyframe, None = all -1; centre_after [K, 3] or None; centres "resident" / "interleaved" / "poses_first";
        scale_factors given = the normals pass runs.  Returns dict(pos [n, 3], status [n]) plus normal, min_distance, max_distance
        with scale_factors."""
        corr, out, _keep = correction(kf_slots, before, after, self.n_points if slots is None else None, slots, corrector, arithmetic,
                                      centre_after, centres, scale_factors)
        check(lib().ydorb_mapdb_correct(self._h, C.byref(corr)))
        return out

    # ------------------------------------------------------------------------------------------------------------ keyframe rows
    def set_keyframe_rows(self, kf_slots, rows):
        """rows[i] = the map-point vector of keyframe slot kf_slots[i] as point slots in keypoint order, -1 = null; an empty row erases."""
        kf_slots = np.ascontiguousarray(kf_slots, np.int32).reshape(-1)
        assert len(rows) == len(kf_slots)
        start, slot = M._csr(rows, np.int32)
        check(lib().ydorb_mapdb_set_keyframe_rows(self._h, _p(kf_slots), len(kf_slots), _p(start), _p(slot)))

    def set_row_entries(self, kf_slot, idx, point_slot):
        kf_slot, idx, point_slot = (np.ascontiguousarray(a, np.int32).reshape(-1) for a in (kf_slot, idx, point_slot))
        assert len(kf_slot) == len(idx) == len(point_slot)
        check(lib().ydorb_mapdb_set_row_entries(self._h, _p(kf_slot), _p(idx), _p(point_slot), len(kf_slot)))

    def row_stats(self):
        s = YdMapDbRowStats()
        check(lib().ydorb_mapdb_row_stats(self._h, C.byref(s)))
        return {name: int(getattr(s, name)) for name, _ in YdMapDbRowStats._fields_}

    def export_rows(self):
        """The device's rows read back: one int32 array per keyframe slot 0 .. n_keyframes-1."""
        k, n = self.n_keyframes, self.row_stats()["n_entries"]
        start, slot = np.zeros(k + 1, np.int32), np.zeros(max(n, 1), np.int32)
        check(lib().ydorb_mapdb_export_rows(self._h, _p(start), _p(slot)))
        assert int(start[-1]) == n
        return [slot[start[i]:start[i + 1]].copy() for i in range(k)]

    def points_of_keyframes(self, kf_slots, seen_points=None, capacity=None):
        """ydorb_mapdb_points_of_keyframes.  capacity None = what always fits.  Returns dict(slots, seen, count, status); slots / seen
        are empty when status is 1."""
        kf_slots = np.ascontiguousarray(kf_slots, np.int32).reshape(-1)
        seen = np.zeros(0, np.int32) if seen_points is None else np.ascontiguousarray(seen_points, np.int32).reshape(-1)
        if capacity is None:
            capacity = self.n_points
        out, flag = np.full(max(capacity, 1), -7, np.int32), np.full(max(capacity, 1), 7, np.uint8)
        count, status = C.c_int32(-1), C.c_uint8(9)
        check(lib().ydorb_mapdb_points_of_keyframes(self._h, _p(kf_slots), len(kf_slots), _p(seen) if len(seen) else None, len(seen), capacity,
                                                    _p(out), _p(flag), C.byref(count), C.byref(status)))
        n = count.value if status.value == 0 else 0
        return dict(slots=out[:n], seen=flag[:n], count=count.value, status=status.value, raw_slots=out, raw_seen=flag)

    def observer_counter(self, lists, capacities=None):
        """ydorb_mapdb_observer_counter.  lists[q] = point slots (-1 allowed).  capacities None = n_keyframes per list.  Returns
        dict(kf, weight [per list], counts, status, point_bad [per list])."""
        nl = len(lists)
        ls, idx = M._csr(lists, np.int32)
        caps = [self.n_keyframes] * nl if capacities is None else list(capacities)
        os_ = np.concatenate([[0], np.cumsum(caps)]).astype(np.int32)
        tot = int(os_[-1])
        kf, w = np.full(max(tot, 1), -7, np.int32), np.full(max(tot, 1), -7, np.int32)
        counts, status, pbad = np.zeros(max(nl, 1), np.int32), np.zeros(max(nl, 1), np.uint8), np.zeros(max(len(idx), 1), np.uint8)
        check(lib().ydorb_mapdb_observer_counter(self._h, nl, _p(ls), _p(idx), _p(os_), _p(kf), _p(w), _p(counts), _p(status), _p(pbad)))
        take = [int(counts[q]) if status[q] == 0 else 0 for q in range(nl)]
        return dict(kf=[kf[os_[q]:os_[q] + take[q]] for q in range(nl)], weight=[w[os_[q]:os_[q] + take[q]] for q in range(nl)],
                    counts=counts[:nl], status=status[:nl], point_bad=[pbad[ls[q]:ls[q + 1]] for q in range(nl)], raw_kf=kf, raw_weight=w)

    # ------------------------------------------------------------------------------------------------------------ local BA graph
    def local_ba_graph(self, kf_slots, inv_level_sigma2):
        """ydorb_mapdb_local_ba_graph: the flat graph of localBundleAdjust for the local keyframes kf_slots, assembled
        on the device.  inv_level_sigma2 [8].  Returns numpy arrays copied out of the handle's memory: dict(n_local, n_fixed, pose_kf,
        pose_fixed [n_poses], point_slot, point_status [n_points], points [n_points, 3] float64, edge_pose, edge_point, edge_kf, edge_idx
        [n_edges], edge_meas [n_edges, 3], edge_inv_sigma2 [n_edges])."""
        kf_slots = np.ascontiguousarray(kf_slots, np.int32).reshape(-1)
        sig = np.ascontiguousarray(inv_level_sigma2, np.float32).reshape(-1)
        assert len(sig) == 8
        g = YdLocalBaGraph()
        check(lib().ydorb_mapdb_local_ba_graph(self._h, _p(kf_slots), len(kf_slots), _p(sig), C.byref(g)))
        P = g.problem

        def take(ptr, dtype, *shape):
            n = int(np.prod(shape))
            if n == 0:
                return np.zeros(shape, dtype)
            return np.frombuffer(C.string_at(ptr, n * np.dtype(dtype).itemsize), dtype).reshape(shape).copy()
        return dict(n_local=g.n_local, n_fixed=g.n_fixed, pose_kf=take(g.pose_kf, np.int32, P.n_poses), pose_fixed=take(P.pose_fixed, np.uint8, P.n_poses),
                    point_slot=take(g.point_slot, np.int32, P.n_points), point_status=take(g.point_status, np.uint8, P.n_points),
                    points=take(P.points, np.float64, P.n_points, 3), edge_pose=take(P.edge_pose, np.int32, P.n_edges),
                    edge_point=take(P.edge_point, np.int32, P.n_edges), edge_kf=take(g.edge_kf, np.int32, P.n_edges),
                    edge_idx=take(g.edge_idx, np.int32, P.n_edges), edge_meas=take(P.edge_meas, np.float64, P.n_edges, 3),
                    edge_inv_sigma2=take(P.edge_inv_sigma2, np.float64, P.n_edges))

    def lba_stats(self):
        s = YdMapDbLbaStats()
        check(lib().ydorb_mapdb_lba_stats(self._h, C.byref(s)))
        return {name: getattr(s, name) for name, _ in YdMapDbLbaStats._fields_}

    def lba_set_profiling(self, on=True):
        """Event pairs round the phases of every later local_ba_graph call; lba_stats() then carries last_ms_*."""
        check(lib().ydorb_mapdb_lba_set_profiling(self._h, int(bool(on))))

    # ------------------------------------------------------------------------------------------------------------ resident descriptors
    def reserve_descriptors(self, view_capacity, descriptor_capacity):
        """Initial capacities of the view pool (views) and the descriptor pool (descriptors); both pools must be empty."""
        check(lib().ydorb_mapdb_reserve_descriptors(self._h, view_capacity, descriptor_capacity))

    def set_keyframe_descriptors(self, kf_slots, blocks):
        """blocks[i] = the descriptor matrix [n_k, 32] uint8 of keyframe slot kf_slots[i] in keypoint order; an empty block erases."""
        kf_slots = np.ascontiguousarray(kf_slots, np.int32).reshape(-1)
        assert len(blocks) == len(kf_slots)
        blocks = [np.ascontiguousarray(b, np.uint8).reshape(-1, 32) for b in blocks]
        start = np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).astype(np.int32)
        desc = np.ascontiguousarray(np.concatenate(blocks + [np.zeros((1, 32), np.uint8)]))
        check(lib().ydorb_mapdb_set_keyframe_descriptors(self._h, _p(kf_slots), len(kf_slots), _p(start), _p(desc)))

    def set_point_views(self, slots, views):
        """views[i] = the places point slots[i] is seen, [m, 2] int32 (keyframe slot, keypoint index) in the observation container's
        order; an empty list erases."""
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        assert len(views) == len(slots)
        views = [np.ascontiguousarray(v, np.int32).reshape(-1, 2) for v in views]
        start = np.concatenate([[0], np.cumsum([len(v) for v in views])]).astype(np.int32)
        flat = np.concatenate(views + [np.zeros((1, 2), np.int32)])
        kf, idx = np.ascontiguousarray(flat[:, 0]), np.ascontiguousarray(flat[:, 1])
        check(lib().ydorb_mapdb_set_point_views(self._h, _p(slots), len(slots), _p(start), _p(kf), _p(idx)))

    def distinctive_descriptors(self, slots):
        """ydorb_mapdb_distinctive_descriptors for the named slots.  Returns dict(best [n], best_view [n, 2], desc [n, 32], status [n])."""
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        n = len(slots)
        m = max(n, 1)
        best, view = np.full(m, -7, np.int32), np.full((m, 2), -7, np.int32)
        desc, st = np.full((m, 32), 7, np.uint8), np.full(m, 9, np.uint8)
        check(lib().ydorb_mapdb_distinctive_descriptors(self._h, _p(slots), n, _p(best), _p(view), _p(desc), _p(st)))
        return dict(best=best[:n], best_view=view[:n], desc=desc[:n], status=st[:n])

    def desc_stats(self):
        s = YdMapDbDescStats()
        check(lib().ydorb_mapdb_desc_stats(self._h, C.byref(s)))
        return {name: int(getattr(s, name)) for name, _ in YdMapDbDescStats._fields_}

    def export_views(self):
        """The device's views read back: one [m, 2] int32 array per point slot 0 .. n_points-1."""
        n, N = self.n_points, self.desc_stats()["n_views"]
        start, kf, idx = np.zeros(n + 1, np.int32), np.zeros(max(N, 1), np.int32), np.zeros(max(N, 1), np.int32)
        check(lib().ydorb_mapdb_export_views(self._h, _p(start), _p(kf), _p(idx)))
        assert int(start[-1]) == N
        return [np.stack([kf[start[i]:start[i + 1]], idx[start[i]:start[i + 1]]], axis=1) for i in range(n)]

    def export_descriptors(self):
        """The device's blocks read back: one [n_k, 32] uint8 array per keyframe slot 0 .. n_keyframes-1."""
        k, N = self.n_keyframes, self.desc_stats()["n_descriptors"]
        start, desc = np.zeros(k + 1, np.int32), np.zeros((max(N, 1), 32), np.uint8)
        check(lib().ydorb_mapdb_export_descriptors(self._h, _p(start), _p(desc)))
        assert int(start[-1]) == N
        return [desc[start[i]:start[i + 1]].copy() for i in range(k)]

    # ------------------------------------------------------------------------------------------------------------ point attributes
    def enable_attributes(self):
        """Turns the resident point attributes on; calling it twice is fine."""
        check(lib().ydorb_mapdb_enable_attributes(self._h))

    def set_point_attributes(self, slots, normal=None, min_distance=None, max_distance=None, desc=None):
        """Stages normal [n, 3], min_distance, max_distance [n] (the raw values; all three or none) and / or desc [n, 32] of the slots."""
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        n = len(slots)
        normal = None if normal is None else np.ascontiguousarray(normal, np.float32).reshape(n, 3)
        mn, mx = (None if a is None else np.ascontiguousarray(a, np.float32).reshape(n) for a in (min_distance, max_distance))
        desc = None if desc is None else np.ascontiguousarray(desc, np.uint8).reshape(n, 32)
        check(lib().ydorb_mapdb_set_point_attributes(self._h, _p(slots), n, _p(normal), _p(mn), _p(mx), _p(desc)))

    def export_attributes(self):
        """The device's attributes read back: dict(normal [n, 3], min_distance, max_distance [n], desc [n, 32], flags [n])."""
        n = self.n_points
        m = max(n, 1)
        normal, mn, mx = np.zeros((m, 3), np.float32), np.zeros(m, np.float32), np.zeros(m, np.float32)
        desc, flags = np.zeros((m, 32), np.uint8), np.zeros(m, np.uint8)
        check(lib().ydorb_mapdb_export_attributes(self._h, _p(normal), _p(mn), _p(mx), _p(desc), _p(flags)))
        return dict(normal=normal[:n], min_distance=mn[:n], max_distance=mx[:n], desc=desc[:n], flags=flags[:n])

    def attr_stats(self):
        s = YdMapDbAttrStats()
        check(lib().ydorb_mapdb_attr_stats(self._h, C.byref(s)))
        return {name: int(getattr(s, name)) for name, _ in YdMapDbAttrStats._fields_}

    def frustum_cull(self, views, lists, skips):
        """ydorb_mapdb_frustum_cull: views [YdFrustumView], per view a list of point slots and its skip bytes.  Returns per view
        dict(rows [m] TRACK_DTYPE, status [m] uint8, n_in_view), as ydorbslam_amd.frustum.frustum_cull does."""
        from ._lib import YdFrustumView
        from .frustum import TRACK_DTYPE
        F = len(views)
        v = (YdFrustumView * max(F, 1))(*views)
        idx = [np.asarray(a, np.int32).reshape(-1) for a in lists]
        sk = [np.asarray(a, np.uint8).reshape(-1) for a in skips]
        assert len(idx) == len(sk) == F and all(len(a) == len(b) for a, b in zip(idx, sk))
        start = np.concatenate([[0], np.cumsum([len(a) for a in idx])]).astype(np.int32)
        slots = np.ascontiguousarray(np.concatenate(idx + [np.zeros(0, np.int32)]))
        skip = np.ascontiguousarray(np.concatenate(sk + [np.zeros(0, np.uint8)]))
        L = int(start[-1])
        rows, status, n_in = np.zeros(max(L, 1), TRACK_DTYPE), np.full(max(L, 1), 9, np.uint8), np.zeros(max(F, 1), np.int32)
        check(lib().ydorb_mapdb_frustum_cull(self._h, C.cast(v, C.c_void_p), F, _p(start), _p(slots), _p(skip), _p(rows), _p(status), _p(n_in)))
        return [dict(rows=rows[start[f]:start[f + 1]].copy(), status=status[start[f]:start[f + 1]].copy(), n_in_view=int(n_in[f])) for f in range(F)]

    def search_local_points(self, matcher, frame, view, point_slots, skip, th, taken=None, assigned=None):
        """ydorb_mapdb_search_local_points on an OrbMatcher (ydorbslam_amd.matcher; its ratio is used) and one of its frames.  Returns
        the dict of ydorbslam_amd.frustum.search_local_points; assigned holds list indices into point_slots."""
        from .frustum import TRACK_DTYPE
        slots = np.ascontiguousarray(point_slots, np.int32).reshape(-1)
        skip = np.ascontiguousarray(skip, np.uint8).reshape(-1)
        n = len(slots)
        assert len(skip) == n
        taken = np.zeros(frame.n, np.uint8) if taken is None else np.ascontiguousarray(taken, np.uint8).copy()
        assigned = np.full(frame.n, -1, np.int32) if assigned is None else np.ascontiguousarray(assigned, np.int32).copy()
        rows, status = np.zeros(max(n, 1), TRACK_DTYPE), np.full(max(n, 1), 9, np.uint8)
        n_to, n_m = C.c_int32(-1), C.c_int32(-1)
        fv = frame.c()
        check(lib().ydorb_mapdb_search_local_points(self._h, matcher._h, C.byref(fv), C.byref(view), _p(slots), n, _p(skip), float(th), matcher.ratio,
                                                    _p(taken), _p(assigned), _p(rows), _p(status), C.byref(n_to), C.byref(n_m)))
        return dict(n_to_match=n_to.value, n_matches=n_m.value, assigned=assigned, taken=taken, rows=rows[:n], status=status[:n])

    # ------------------------------------------------------------------------------------------------------------ keyframe features
    def enable_features(self):
        """Turns the resident keyframe features on; calling it twice is fine."""
        check(lib().ydorb_mapdb_enable_features(self._h))

    def set_keyframe_features(self, kf_slots, kps, right_x=None):
        """Stages the features of the keyframes: kps = one KP_DTYPE array per slot, right_x = one float32 array per slot or None
        (monocular: every entry is stored as -1).  An empty array erases a keyframe's features."""
        kf_slots = np.ascontiguousarray(kf_slots, np.int32).reshape(-1)
        kps = [np.ascontiguousarray(a, KP_DTYPE).reshape(-1) for a in kps]
        assert len(kps) == len(kf_slots)
        start = np.concatenate([[0], np.cumsum([len(a) for a in kps])]).astype(np.int32)
        flat = np.ascontiguousarray(np.concatenate(kps + [np.zeros(0, KP_DTYPE)]))
        rx = None
        if right_x is not None:
            right_x = [np.ascontiguousarray(a, np.float32).reshape(-1) for a in right_x]
            assert [len(a) for a in right_x] == [len(a) for a in kps]
            rx = np.ascontiguousarray(np.concatenate(right_x + [np.zeros(0, np.float32)]))
        check(lib().ydorb_mapdb_set_keyframe_features(self._h, _p(kf_slots), len(kf_slots), _p(start), _p(flat), _p(rx)))

    def export_features(self):
        """The device's features read back: per keyframe slot 0 .. n_keyframes-1 a (kps [n_k] KP_DTYPE, right_x [n_k]) pair."""
        k, N = self.n_keyframes, self.feat_stats()["n_features"]
        start, kps, rx = np.zeros(k + 1, np.int32), np.zeros(max(N, 1), KP_DTYPE), np.zeros(max(N, 1), np.float32)
        check(lib().ydorb_mapdb_export_features(self._h, _p(start), _p(kps), _p(rx)))
        assert int(start[-1]) == N
        return [(kps[start[i]:start[i + 1]].copy(), rx[start[i]:start[i + 1]].copy()) for i in range(k)]

    def feat_stats(self):
        s = YdMapDbFeatStats()
        check(lib().ydorb_mapdb_feat_stats(self._h, C.byref(s)))
        return {name: int(getattr(s, name)) for name, _ in YdMapDbFeatStats._fields_}

    def fuse_search(self, matcher, targets, lists, skips):
        """ydorb_mapdb_fuse_search on an OrbMatcher (ydorbslam_amd.matcher): targets [YdFuseTarget], per target a list of point slots and
        its skip bytes.  Returns per target dict(best_idx [m] int32, status [m] uint8, n_found, target_status)."""
        T = len(targets)
        t = (YdFuseTarget * max(T, 1))(*targets)
        idx = [np.asarray(a, np.int32).reshape(-1) for a in lists]
        sk = [np.asarray(a, np.uint8).reshape(-1) for a in skips]
        assert len(idx) == len(sk) == T and all(len(a) == len(b) for a, b in zip(idx, sk))
        start = np.concatenate([[0], np.cumsum([len(a) for a in idx])]).astype(np.int32)
        slots = np.ascontiguousarray(np.concatenate(idx + [np.zeros(0, np.int32)]))
        skip = np.ascontiguousarray(np.concatenate(sk + [np.zeros(0, np.uint8)]))
        L = int(start[-1])
        best, status = np.full(max(L, 1), -7, np.int32), np.full(max(L, 1), 9, np.uint8)
        n_found, t_status = np.full(max(T, 1), -7, np.int32), np.full(max(T, 1), 9, np.uint8)
        check(lib().ydorb_mapdb_fuse_search(self._h, matcher._h, C.cast(t, C.c_void_p), T, _p(start), _p(slots), _p(skip), _p(best), _p(status),
                                            _p(n_found), _p(t_status)))
        return [dict(best_idx=best[start[f]:start[f + 1]].copy(), status=status[start[f]:start[f + 1]].copy(), n_found=int(n_found[f]),
                     target_status=int(t_status[f])) for f in range(T)]

    # ------------------------------------------------------------------------------------------------------------ BoW feature vectors
    def enable_bow(self):
        """Turns the resident BoW feature vectors on; calling it twice is fine."""
        check(lib().ydorb_mapdb_enable_bow(self._h))

    def set_keyframe_bow(self, kf_slots, bows):
        """Stages the feature vectors of the keyframes: bows[i] = [m, 2] (node id, feature index) in map order, nodes ascending.  An
        empty array erases."""
        kf_slots = np.ascontiguousarray(kf_slots, np.int32).reshape(-1)
        bows = [np.asarray(b, np.int64).reshape(-1, 2) for b in bows]
        assert len(bows) == len(kf_slots)
        start = np.concatenate([[0], np.cumsum([len(b) for b in bows])]).astype(np.int32)
        flat = np.concatenate(bows + [np.zeros((0, 2), np.int64)])
        assert not len(flat) or (0 <= flat[:, 0].min() and flat[:, 0].max() < 2 ** 32)
        node, feat = np.ascontiguousarray(flat[:, 0].astype(np.uint32)), np.ascontiguousarray(np.clip(flat[:, 1], -2 ** 31, 2 ** 31 - 1).astype(np.int32))
        check(lib().ydorb_mapdb_set_keyframe_bow(self._h, _p(kf_slots), len(kf_slots), _p(start), _p(node), _p(feat)))

    def export_bow(self):
        """The device's feature vectors read back: one [m, 2] int64 array (node id, feature index) per keyframe slot 0 .. n_keyframes-1."""
        k, N = self.n_keyframes, self.bow_stats()["n_entries"]
        start, node, feat = np.zeros(k + 1, np.int32), np.zeros(max(N, 1), np.uint32), np.zeros(max(N, 1), np.int32)
        check(lib().ydorb_mapdb_export_bow(self._h, _p(start), _p(node), _p(feat)))
        assert int(start[-1]) == N
        return [np.stack([node[start[i]:start[i + 1]].astype(np.int64), feat[start[i]:start[i + 1]].astype(np.int64)], axis=1) for i in range(k)]

    def bow_stats(self):
        s = YdMapDbBowStats()
        check(lib().ydorb_mapdb_bow_stats(self._h, C.byref(s)))
        return {name: int(getattr(s, name)) for name, _ in YdMapDbBowStats._fields_}

    def create_new_points(self, matcher, first, neighbours, stereo_only=False, check_orientation=False):
        """ydorb_mapdb_create_new_points on an OrbMatcher: first = a YdCreateView (create_view), neighbours = [YdCreateNeighbour]
        (create_neighbour) in the caller's order.  Returns dict(matched_second [n_nb, n], x3d [n_nb, n, 3], status [n_nb, n],
        n_matches, n_accepted, neighbour_status [n_nb])."""
        nn, n = len(neighbours), int(first.n)
        nb = (YdCreateNeighbour * max(nn, 1))(*neighbours)
        shape = (max(nn, 1), n)   # n == 0: the call gets no output arrays to fill
        matched, x3d, status = np.full(shape, -7, np.int32), np.full(shape + (3,), 7, np.float32), np.full(shape, 9, np.uint8)
        n_m, n_a, nb_st = np.full(max(nn, 1), -7, np.int32), np.full(max(nn, 1), -7, np.int32), np.full(max(nn, 1), 9, np.uint8)
        check(lib().ydorb_mapdb_create_new_points(self._h, matcher._h, C.byref(first), C.cast(nb, C.c_void_p), nn, int(bool(stereo_only)),
                                                  int(bool(check_orientation)), _p(matched) if n else None, _p(x3d) if n else None,
                                                  _p(status) if n else None, _p(n_m), _p(n_a), _p(nb_st)))
        return dict(matched_second=matched[:nn], x3d=x3d[:nn], status=status[:nn], n_matches=n_m[:nn], n_accepted=n_a[:nn], neighbour_status=nb_st[:nn])

    def search_by_bow_keyframes(self, matcher, first_kf_slot, second_kf_slots, n_first, ratio=None, check_orientation=None):
        """ydorb_mapdb_search_by_bow_keyframes on an OrbMatcher (its ratio and check_orientation unless given): searchByBowInTwoKeyFrames
        (first, second_i) for every second keyframe, independently.  Returns dict(matched_second [n_second, n_first], matched_point
        [n_second, n_first], n_matches, pair_status [n_second])."""
        second = np.ascontiguousarray(second_kf_slots, np.int32).reshape(-1)
        ns, n = len(second), int(n_first)
        shape = (max(ns, 1), max(n, 0))
        matched, point = np.full(shape, -7, np.int32), np.full(shape, -7, np.int32)
        n_m, st = np.full(max(ns, 1), -7, np.int32), np.full(max(ns, 1), 9, np.uint8)
        check(lib().ydorb_mapdb_search_by_bow_keyframes(self._h, matcher._h, int(first_kf_slot), _p(second) if ns else None, ns,
                                                        float(matcher.ratio if ratio is None else ratio),
                                                        int(bool(matcher.check_orientation if check_orientation is None else check_orientation)), n,
                                                        _p(matched) if n > 0 else None, _p(point) if n > 0 else None, _p(n_m), _p(st)))
        return dict(matched_second=matched[:ns], matched_point=point[:ns], n_matches=n_m[:ns], pair_status=st[:ns])

    def search_by_bow_frame(self, matcher, kf_slots, kps, desc, valid, fv, ratio=None, check_orientation=None):
        """ydorb_mapdb_search_by_bow_frame on an OrbMatcher: searchByBowInKeyFrameAndFrame(kf_i, frame) for every keyframe, independently.
        The frame: kps [n] KP_DTYPE, desc [n, 32], valid [n] or None (every feature), fv a matcher.FeatureVector.  Returns
        dict(matched_kf_feature [n_kf, n], matched_point [n_kf, n], n_matches, pair_status [n_kf])."""
        slots = np.ascontiguousarray(kf_slots, np.int32).reshape(-1)
        kps = np.ascontiguousarray(kps, KP_DTYPE).reshape(-1)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        valid = None if valid is None else np.ascontiguousarray(valid, np.uint8).reshape(-1)
        nk, n = len(slots), len(kps)
        assert len(desc) == n and (valid is None or len(valid) == n)
        frame = YdBowSide(_p(kps) if n else None, _p(desc) if n else None, _p(valid) if valid is not None and n else None, n, fv.c())
        shape = (max(nk, 1), n)
        matched, point = np.full(shape, -7, np.int32), np.full(shape, -7, np.int32)
        n_m, st = np.full(max(nk, 1), -7, np.int32), np.full(max(nk, 1), 9, np.uint8)
        check(lib().ydorb_mapdb_search_by_bow_frame(self._h, matcher._h, _p(slots) if nk else None, nk, C.byref(frame),
                                                    float(matcher.ratio if ratio is None else ratio),
                                                    int(bool(matcher.check_orientation if check_orientation is None else check_orientation)),
                                                    _p(matched) if n else None, _p(point) if n else None, _p(n_m), _p(st)))
        return dict(matched_kf_feature=matched[:nk], matched_point=point[:nk], n_matches=n_m[:nk], pair_status=st[:nk])

    # ------------------------------------------------------------------------------------------------------------ inspection
    def stats(self):
        s = YdMapDbStats()
        check(lib().ydorb_mapdb_stats(self._h, C.byref(s)))
        return {name: int(getattr(s, name)) for name, _ in YdMapDbStats._fields_}

    def export(self):
        """The device's table read back: dict(table [ObservationTable], ref_kf, ref_level, pos, centre)."""
        s = self.stats()
        n, k, N = s["n_points"], s["n_keyframes"], s["n_observations"]
        start, kf, lv = np.zeros(n + 1, np.int32), np.zeros(max(N, 1), np.int32), np.zeros(max(N, 1), np.uint8)
        bad, ref_kf, ref_level = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint8)
        pos, centre = np.zeros((max(n, 1), 3), np.float32), np.zeros((max(k, 1), 3), np.float32)
        check(lib().ydorb_mapdb_export(self._h, _p(start), _p(kf), _p(lv), _p(bad), _p(ref_kf), _p(ref_level), _p(pos), _p(centre)))
        assert int(start[-1]) == N
        return dict(table=M.ObservationTable.from_arrays(k, start, kf[:N], lv[:N], bad[:n]), ref_kf=ref_kf[:n], ref_level=ref_level[:n], pos=pos[:n],
                    centre=centre[:k])


class _Header:
    """What map_maintenance's wrappers read of a table, answered once per call from the handle."""

    def __init__(self, db):
        self.n_keyframes, self.struct, self._db = db.n_keyframes, C.c_int(0), db

    def span_lengths(self):
        return self._db.span_lengths()


def create_view(kf_slot, depth, Tcw, Ow, fx, fy, cx, cy, b, bf, level_sigma2, scale_factors):
    """A YdCreateView over numpy arrays: Tcw [3, 4], Ow [3]; Rwc = Rcw^T; invfx = 1.0f / fx as the reference stores it.  The struct
    points into `depth`: the returned pair keeps it alive."""
    depth = np.ascontiguousarray(depth, np.float32).reshape(-1)
    Tcw = np.ascontiguousarray(Tcw, np.float32).reshape(3, 4)
    Rwc = np.ascontiguousarray(Tcw[:, :3].T)
    s2, sf = (np.ascontiguousarray(a, np.float32).reshape(-1) for a in (level_sigma2, scale_factors))
    assert len(s2) == len(sf)
    L = len(sf)
    pad = lambda a: (C.c_float * 8)(*([float(x) for x in a[:8]] + [0.0] * max(8 - L, 0)))
    v = YdCreateView(kf_slot=int(kf_slot), n=len(depth), depth=_p(depth) if len(depth) else None, Tcw=(C.c_float * 12)(*Tcw.reshape(-1)),
                     Rwc=(C.c_float * 9)(*Rwc.reshape(-1)), Ow=(C.c_float * 3)(*np.asarray(Ow, np.float32).reshape(-1)), fx=fx, fy=fy, cx=cx, cy=cy,
                     invfx=float(np.float32(1.0) / np.float32(fx)), invfy=float(np.float32(1.0) / np.float32(fy)), b=b, bf=bf,
                     level_sigma2=pad(s2), scale_factors=pad(sf), n_levels=L)
    return v, depth


def create_neighbour(view, F, ex, ey, ratio_factor):
    return YdCreateNeighbour(view=view, F=(C.c_float * 9)(*np.asarray(F, np.float32).reshape(-1)), ex=ex, ey=ey, ratio_factor=ratio_factor)
