"""Time of the search of LocalMapping::searchInNeighbors, host to host at the C entry points, on a workload of its shape: one new
keyframe of 1000 / 2000 features and its map points against 10 / 30 neighbours of as many features (tests/mapdb_fuse_support.Scene),
both directions: the new keyframe's points into every neighbour (one target per neighbour), then the neighbours' points into the new
keyframe (one target).  Three variants:
  (i)   flat       per target a host gather of the listed points (a numpy index over map-wide arrays), pass 1 by the test restatement
                   (tests/fuse_ref, one CPU thread; the adapter's loop over MapPoint objects is not measured) and one ydorb_fuse_search /
                   ydorb_window_search with the keyframe's keypoints, descriptors and right coordinates uploaded; each part timed on
                   its own;
  (ii)  resident   ydorb_mapdb_fuse_search, one call per direction, nothing staged;
  (iii) restaged   the new keyframe's features, descriptor block and its points' attributes staged first (timed on its own), then the
                   same two calls.
The three alternate within each of 30 repetitions; their results are compared exactly before and after.  Bytes uploaded per variant are
counted from the arguments (flat) and from the arguments plus the handle's sync counters (resident).  Prints one JSON line.
With --profile it only repeats variant (ii) on the largest case, for a kernel trace of its launches."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mapdb_fuse_support as R  # noqa: E402
import ydorbslam_amd as y  # noqa: E402

REPS = 30
f32 = np.float32


def med(v):
    return [round(float(x) * 1e3, 4) for x in (np.median(v), min(v), max(v))]


def case(m, n_feat, n_nb, reps=REPS, only_resident=False):
    s = R.Scene(seed=n_feat + n_nb, n_kf=n_nb + 1, n_feat=n_feat, n_points=2 * n_feat)
    db = y.MapDb(0, 2 * n_feat, n_nb + 1, 8 * n_feat)
    s.load(db)
    own = np.arange(0, n_feat, dtype=np.int32)            # the new keyframe's points
    theirs = np.arange(n_feat, 2 * n_feat, dtype=np.int32)   # the neighbours'
    zeros = np.zeros(n_feat, np.uint8)
    dirs = [([s.target(k) for k in range(1, n_nb + 1)], [own] * n_nb, [zeros] * n_nb), ([s.target(0)], [theirs], [zeros])]
    mp = R.exported_map(db)
    feats, blocks = db.export_features(), db.export_descriptors()
    part = dict(gather=[], pass1=[], flat_search=[], flat=[], resident=[], stage=[], restaged=[])

    def flat():
        out, t_g, t_p, t_s = [], 0.0, 0.0, 0.0
        for targets, lists, skips in dirs:
            for G, slots, skip in zip(targets, lists, skips):
                t0 = time.perf_counter()
                rows = [mp[k][slots] for k in ("pos", "bad", "normal", "mn", "mx", "desc", "flags")]   # what the flat call's host side reads per point
                t1 = time.perf_counter()
                r = R.ref_queries(mp, [G], [slots], [skip])[0]
                t2 = time.perf_counter()
                kps, rx = feats[G.kf_slot]
                V = G.view
                n, best = m.fuse_search(y.FrameView(kps, blocks[G.kf_slot], (V.min_x, V.max_x, V.min_y, V.max_y), rx), r["queries"], r["qdesc"],
                                        np.array(G.inv_sigma2[:], f32), G.max_dist)
                t3 = time.perf_counter()
                t_g, t_p, t_s = t_g + t1 - t0, t_p + t2 - t1, t_s + t3 - t2
                out.append((n, best, r["status"], len(rows)))
        part["gather"].append(t_g); part["pass1"].append(t_p); part["flat_search"].append(t_s); part["flat"].append(t_g + t_p + t_s)
        return out

    def resident(key="resident"):
        t0 = time.perf_counter()
        out = [g for d in dirs for g in db.fuse_search(m, *d)]
        part[key].append(time.perf_counter() - t0)
        return out

    g = np.flatnonzero((s.flags[own] & 1) != 0).astype(np.int32)
    d = np.flatnonzero((s.flags[own] & 2) != 0).astype(np.int32)

    staged = []

    def restaged():
        t0 = time.perf_counter()
        s.load_keyframes(db, [0])
        db.set_point_attributes(g, s.normal[g], s.mn[g], s.mx[g], None)
        db.set_point_attributes(d, desc=s.pdesc[d])
        t1 = time.perf_counter()
        out = db.fuse_search(m, *dirs[0])
        t2 = time.perf_counter()                           # the first call applied what was staged: its counters, read outside the timing
        staged.append(db.feat_stats()["last_feat_sync_bytes"] + db.desc_stats()["last_desc_sync_bytes"] + db.attr_stats()["last_attr_sync_bytes"])
        t3 = time.perf_counter()
        out = out + db.fuse_search(m, *dirs[1])
        part["stage"].append(t1 - t0); part["restaged"].append((t2 - t0) + (time.perf_counter() - t3))
        return out

    def check():
        a, b, c = flat(), resident(), restaged()
        for x, u, v in zip(a, b, c):
            for w in (u, v):
                assert w["target_status"] == 0 and w["n_found"] == x[0] and np.array_equal(w["best_idx"], x[1]) and np.array_equal(w["status"], x[2])
        return sum(x[0] for x in a)

    if only_resident:
        for _ in range(reps):
            resident()
        db.close()
        return dict(resident_ms=med(part["resident"]))
    found = check()
    for _ in range(3):
        flat(); resident(); restaged()
    for v in part.values():
        v.clear()
    for _ in range(reps):                                  # the variants alternate within each repetition
        flat(); resident(); restaged()
    out = {k + "_ms": med(v) for k, v in part.items()}
    assert check() == found
    L1, L2 = n_nb * n_feat, n_feat
    call_bytes = (n_nb + 1) * C.sizeof(y._lib.YdFuseTarget) + 4 * (n_nb + 3) + 5 * (L1 + L2)
    out["upload_bytes"] = dict(flat=(n_nb + 1) * n_feat * (28 + 32 + 4) + (L1 + L2) * (40 + 32), resident=call_bytes, restaged=call_bytes + int(max(staged)))
    out["list_entries"], out["found"] = L1 + L2, found
    db.close()
    return out


def main():
    m = y.OrbMatcher(0.6, True)
    if "--profile" in sys.argv[1:]:
        print(json.dumps({"metric": "fuse_search_profile", "feat2000_nb30": case(m, 2000, 30, reps=20, only_resident=True)}))
        return
    out = {"metric": "search_in_neighbors_ms", "reps": REPS, "cases": {}}
    for n_feat in (1000, 2000):
        for n_nb in (10, 30):
            out["cases"]["feat%d_nb%d" % (n_feat, n_nb)] = case(m, n_feat, n_nb)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
