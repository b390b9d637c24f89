"""Time of the BoW searches of a loop-closing or relocalisation round, host to host at the C entry point: keyframes
of 1 000 and 2 000 features over 200 vocabulary nodes (tests/mapdb_bowsearch_support.Scene), 1, 5 and 20 candidates, both forms.  Two
ways alternate within each of 15 repetitions after a warm-up, their results compared exactly before and after the timed loop:
  (i)  resident   one ydorb_mapdb_search_by_bow_keyframes / ydorb_mapdb_search_by_bow_frame call with nothing staged;
  (ii) flat       the loop of N ydorb_search_by_bow calls on the same data, the YdBowSide structs and the valid bytes prepared outside
                  the timing (the adapters build them per call from the map-point vectors: this understates the flat loop).
Per case also the bytes up and down and the launches and synchronisations of one resident call (ydorb_matcher_bow_search_stats) and
of the flat loop (counted from bowSearch in orb_matcher.hip: nine copies up, two down, two launches and one synchronisation per call),
and, in a run of its own with the matcher's profiling switch, the device time of join + gather, resolve and emit.  Prints one JSON line."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mapdb_bowsearch_support as B  # noqa: E402
import ydorbslam_amd as y  # noqa: E402
from ydorbslam_amd._lib import YdBowSide, lib  # noqa: E402

REPS = 15
FEATURES = (1000, 2000)
CANDIDATES = (1, 5, 20)
RATIO, ORI = 0.75, 1


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def med(v):
    return [round(float(x) * 1e3, 4) for x in (np.median(v), min(v), max(v))]


def nodes200(point, kf):
    return (point % 200).astype(np.uint32) * 5 + 2


def flat_bytes(A, Bs, va, mode):
    """What bowSearch uploads and reads back for one pair."""
    bucket = dict(zip(*np.unique(Bs["bow"][:, 0], return_counts=True)))
    nq = sum(1 for node, f in A["bow"] if va[f] and node in bucket)
    n_a, n_b = len(A["kps"]), len(Bs["kps"])
    up = 32 * n_a + 32 * n_b + 28 * n_b + 4 * len(Bs["bow"]) + (n_b if mode == 4 else 0) + 16 * nq
    return up, 12 + 4 * max(nq, n_b)


def case(scene, db, m, arrays, mode, n_cand):
    L = lib()
    cands = np.ascontiguousarray(scene.slots[1:1 + n_cand], np.int32)
    first = scene.slots[0]
    n_out = len(arrays["kf"][first]["kps"]) if mode == 4 else len(scene.frame["kps"])
    matched, point = np.zeros((n_cand, n_out), np.int32), np.zeros((n_cand, n_out), np.int32)
    counts, status = np.zeros(n_cand, np.int32), np.zeros(n_cand, np.uint8)
    keep = []

    def side(S, valid):
        kps, desc = np.ascontiguousarray(S["kps"]), np.ascontiguousarray(S["desc"])
        fv = y.FeatureVector(*B.csr(S["bow"]))
        keep.extend([kps, desc, valid, fv])
        return YdBowSide(_p(kps), _p(desc), None if valid is None else _p(valid), len(kps), fv.c())
    frame = side(scene.frame, None)
    pairs, up, down = [], 0, 0
    for c in cands:
        A = arrays["kf"][first if mode == 4 else c]
        Bs = arrays["kf"][c] if mode == 4 else scene.frame
        va = B.good(A["row"], arrays["bad"])
        pairs.append((side(A, va), side(Bs, B.good(Bs["row"], arrays["bad"])) if mode == 4 else frame))
        u, d = flat_bytes(A, Bs, va, mode)
        up, down = up + u, down + d
    flat_out, flat_n = np.zeros((n_cand, n_out), np.int32), C.c_int32(0)
    flat_counts = np.zeros(n_cand, np.int32)
    part = dict(resident=[], flat=[])

    def resident():
        t0 = time.perf_counter()
        if mode == 4:
            rc = L.ydorb_mapdb_search_by_bow_keyframes(db._h, m._h, first, _p(cands), n_cand, RATIO, ORI, n_out, _p(matched), _p(point), _p(counts), _p(status))
        else:
            rc = L.ydorb_mapdb_search_by_bow_frame(db._h, m._h, _p(cands), n_cand, C.byref(frame), RATIO, ORI, _p(matched), _p(point), _p(counts), _p(status))
        part["resident"].append(time.perf_counter() - t0)
        assert rc == 0

    def flat():
        t0 = time.perf_counter()
        for i, (a, b) in enumerate(pairs):
            rc = L.ydorb_search_by_bow(m._h, mode, C.byref(a), C.byref(b), RATIO, ORI, C.c_void_p(flat_out[i].ctypes.data), C.byref(flat_n))
            flat_counts[i] = flat_n.value
            assert rc == 0
        part["flat"].append(time.perf_counter() - t0)

    def same():
        resident(); flat()
        assert np.array_equal(matched, flat_out) and np.array_equal(counts, flat_counts) and not status.any()

    for _ in range(3):
        same()
    for v in part.values():
        v.clear()
    for _ in range(REPS):
        resident(); flat()
    same()
    for v in part.values():
        del v[-1:]
    st = m.bow_search_stats()
    m.set_profiling(True)                                        # a run of its own: the event pairs cost stream time
    for _ in range(REPS):
        resident()
    ms = m.bow_search_stats()["ms"]
    m.set_profiling(False)
    del part["resident"][-REPS:]
    out = {k + "_ms": med(v) for k, v in part.items()}
    out.update(speedup=round(out["flat_ms"][0] / out["resident_ms"][0], 3), matches=int(counts.sum()),
               resident=dict(bytes_up=st["bytes_up"], bytes_down=st["bytes_down"], launches=st["launches"], synchronisations=st["synchronisations"]),
               flat=dict(bytes_up=int(up), bytes_down=int(down), launches=2 * n_cand, synchronisations=n_cand, copies=11 * n_cand),
               gpu_ms=dict(zip(("join_gather", "resolve", "emit"), [round(float(v), 4) for v in ms])))
    return out


def main():
    out = {"metric": "bow_search_ms", "reps": REPS, "ratio": RATIO, "check_orientation": ORI, "cases": {}}
    for n in FEATURES:
        scene = B.Scene(seed=n, n=n, n_cand=max(CANDIDATES), nodes=nodes200)
        db = y.MapDb(0, scene.n_points + 8, 32, 1024)
        scene.load(db)
        arrays = B.gather(db)
        m = y.OrbMatcher(RATIO, bool(ORI))
        for mode, name in ((4, "keyframes"), (3, "frame")):
            for n_cand in CANDIDATES:
                out["cases"]["%s_n%d_cand%d" % (name, n, n_cand)] = case(scene, db, m, arrays, mode, n_cand)
        m.close()
        db.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
