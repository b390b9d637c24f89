"""Test support of ydorb_mapdb_search_by_bow_keyframes / ydorb_mapdb_search_by_bow_frame: the scenes and the
reference.  A scene is a first keyframe, candidate keyframes of different feature counts and a frame that all see the same base
features: most rows name a map point, a tenth of the points are flagged bad, a few rows name a slot never set, and a few "twin"
features per keyframe (same node, descriptors one or two bits apart) make the ratio test reject.  The reference is the matcher
oracle's search_by_bow per pair on arrays gathered in Python from the handle's exports, with `valid` computed in Python by the rule of
the header: the row entry is >= 0, below the number of point slots, and its bad flag is clear (a slot never set reads as bad).
analyse() restates one pair as a brute-force Python loop that also says why each query ended as it did; the CPU test holds it to the
oracle and reads the scene conditions from it."""
import os

import numpy as np

from mapdb_tri_support import bucket_nodes, default_nodes, one_node
from triangulate_support import ROOT

f32 = np.float32
CHECK_SRC = os.path.join(ROOT, "tests", "cpu_harness", "mapdb_bowsearch_check.cpp")
PAIR_STATUS = {"ok": 0, "no_features": 1, "no_block": 2, "no_bow": 3, "length_mismatch": 4, "bow_index": 5}
POOL_PER_PAIR = 1 << 14   # the records a fresh matcher holds per pair (c_api.h): more than that forces the replay
RESOLVE_WINDOW = 512      # kResolveWindow of match_kernels.hip.h
RATIOS = (0.6, 0.75, 0.9)


def end_nodes(point, kf):
    """Both ends of the join's binary search, for both forms: the first keyframe (the A side of mode 4) files a twelfth of its features
    under node 0 and another under 999983, the candidates (B in mode 4, A in mode 3) under 1 and 999979, the frame (kf < 0, the B side
    of mode 3) under neither."""
    base = default_nodes(point, kf)
    if kf == 0:
        base = np.where(point % 12 == 0, 0, np.where(point % 12 == 11, 999983, base))
    elif kf > 0:
        base = np.where(point % 12 == 1, 1, np.where(point % 12 == 10, 999979, base))
    return base.astype(np.uint32)


def wide_nodes(point, kf):
    """40 vocabulary nodes: the buckets of 600 features stay near 15, so the 600-feature scene fits a fresh pool."""
    return (point % 40).astype(np.uint32) * 5 + 2


def csr(bow):
    """The oracle's (node ids, node start, feature) triple of a [m, 2] (node, feature) array in map order."""
    ids, counts = np.unique(bow[:, 0], return_counts=True)
    assert np.array_equal(np.repeat(ids, counts), bow[:, 0])
    return ids.astype(np.uint32), np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), bow[:, 1].astype(np.int32)


def good(row, bad):
    """The header's "has a good map point" for every entry of a row; bad [n_points] as exported."""
    row = np.asarray(row, np.int64)
    inside = (row >= 0) & (row < len(bad))
    return (inside & (bad[np.where(inside, row, 0)] == 0)).astype(np.uint8)


class Scene:
    """kfs[0] is the first keyframe, kfs[1:] the candidates; frame is the frame of the frame form.  Each: kps [m] KP_DTYPE, desc
    [m, 32], nodes [m], bow [m, 2] in map order, row [m] point slot or -1; the frame has valid [m] instead of a row.  slots[k] = the
    keyframe's slot.  bad [n_points] = the flags the points are set with, 1 for the slots never set."""

    def __init__(self, seed=21, n=300, n_cand=4, nodes=default_nodes, mapped=0.7, bad=0.1, never_set=5, twins=6, step=7, disjoint=(), seen=0.8):
        from ydorbslam_amd import KP_DTYPE
        rng = np.random.default_rng(seed)
        self.n_points = n + 40                                # slot j = the point of base feature j; the rest belong to features of no base
        self.never = np.sort(rng.choice(self.n_points - 1, never_set, replace=False))
        self.bad = (rng.uniform(size=self.n_points) < bad).astype(np.uint8)
        self.bad[self.n_points - 1] = 0
        self.bad[self.never] = 1
        base = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        octave, angle = rng.integers(0, 8, n), rng.uniform(0, 360, n)
        ok_points = np.flatnonzero(self.bad == 0)

        def side(k, m):
            order = np.concatenate([rng.permutation(n), n + np.arange(m - n)])
            real = order < n
            seen_k = real & (rng.uniform(size=m) < (0.9 if k == 0 else seen))
            kps = np.zeros(m, KP_DTYPE)
            kps["x"], kps["y"], kps["class_id"], kps["size"] = rng.uniform(20, 620, m), rng.uniform(20, 460, m), -1, 31
            kps["octave"] = np.where(real, octave[np.minimum(order, n - 1)], 0)
            turn = np.where(rng.uniform(size=m) < 0.85, 10.0 * max(k, 0), rng.uniform(0, 360, m))   # most features turn with the keyframe
            kps["angle"] = (np.where(real, angle[np.minimum(order, n - 1)], 0.0) + turn) % 360.0
            desc = rng.integers(0, 256, (m, 32), dtype=np.uint8)
            desc[seen_k] = base[order[seen_k]]
            for r in np.flatnonzero(seen_k):
                for bit in rng.integers(0, 256, 3):
                    desc[r, bit // 8] ^= np.uint8(1 << (bit % 8))
            nd = nodes(order.astype(np.int64), k).astype(np.int64)
            if k in disjoint:
                nd = nd + 5000
            has = rng.uniform(size=m) < mapped
            row = np.where(has, np.where(seen_k, np.minimum(order, n - 1), rng.integers(n, self.n_points, m)), -1).astype(np.int32)
            # twins: an unseen feature becomes a near copy of a seen one under the same node, with a good point of its own
            src = rng.permutation(np.flatnonzero(seen_k & has))[:twins]
            dst = rng.permutation(np.flatnonzero(~seen_k))[:len(src)]
            for f, g in zip(src, dst):
                desc[g] = desc[f]
                for bit in rng.integers(0, 256, int(rng.integers(1, 3))):
                    desc[g, bit // 8] ^= np.uint8(1 << (bit % 8))
                nd[g], row[g] = nd[f], int(rng.choice(ok_points))
            from helpers import feature_vector
            fv = feature_vector(nd.astype(np.uint32))
            bow = np.stack([np.repeat(fv[0].astype(np.int64), np.diff(fv[1])), fv[2].astype(np.int64)], axis=1)
            return dict(kps=kps, desc=np.ascontiguousarray(desc), nodes=nd, bow=bow, row=row)

        self.slots = [int(s) for s in rng.permutation(n_cand + 3)[:n_cand + 1]]
        self.kfs = [side(k, n + (step * k if k else 0)) for k in range(n_cand + 1)]
        # a few row entries of every keyframe name a slot never set
        for k in self.kfs:
            at = rng.permutation(np.flatnonzero(k["row"] >= 0))[:3]
            k["row"][at] = rng.choice(self.never, len(at))
        self.frame = side(-1, n + 3)
        self.frame["valid"] = (rng.uniform(size=n + 3) < 0.9).astype(np.uint8)
        del self.frame["row"]

    @property
    def n_cand(self):
        return len(self.kfs) - 1

    def load(self, db, skip=()):
        """Puts the scene into a MapDb; the relations named in `skip` ("rows", "blocks", "features", "bow") stay out."""
        db.enable_features()
        db.enable_bow()
        n_kf = max(self.slots) + 1
        db.set_centres(np.arange(n_kf), np.zeros((n_kf, 3), f32))
        live = np.setdiff1d(np.arange(self.n_points), self.never)
        P = len(live)
        db.set_points(live, [[] for _ in range(P)], [[] for _ in range(P)], self.bad[live], np.zeros(P, np.int32), np.zeros(P, np.uint8), np.zeros((P, 3), f32))
        if "rows" not in skip:
            db.set_keyframe_rows(self.slots, [k["row"] for k in self.kfs])
        if "blocks" not in skip:
            db.set_keyframe_descriptors(self.slots, [k["desc"] for k in self.kfs])
        if "features" not in skip:
            db.set_keyframe_features(self.slots, [k["kps"] for k in self.kfs])
        if "bow" not in skip:
            db.set_keyframe_bow(self.slots, [k["bow"] for k in self.kfs])

    def host_arrays(self):
        """What gather() returns for a handle that holds exactly this scene, without a handle (the CPU test)."""
        n_kf = max(self.slots) + 1
        from ydorbslam_amd import KP_DTYPE
        empty = dict(kps=np.zeros(0, KP_DTYPE), desc=np.zeros((0, 32), np.uint8), row=np.zeros(0, np.int32), bow=np.zeros((0, 2), np.int64))
        kf = [dict(empty) for _ in range(n_kf)]
        for s, k in zip(self.slots, self.kfs):
            kf[s] = dict(kps=k["kps"], desc=k["desc"], row=k["row"], bow=k["bow"])
        return dict(kf=kf, bad=self.bad)

    def frame_args(self, valid=True):
        import ydorbslam_amd as y
        F = self.frame
        return F["kps"], F["desc"], (F["valid"] if valid else None), y.FeatureVector(*csr(F["bow"]))


def gather(db):
    """The arrays of the reference, read from the handle's exports: per keyframe slot kps, desc, row, bow; the points' bad flags."""
    feats, blocks, rows, bows = db.export_features(), db.export_descriptors(), db.export_rows(), db.export_bow()
    bad = db.export()["table"].bad
    return dict(kf=[dict(kps=feats[k][0], desc=blocks[k], row=rows[k], bow=bows[k]) for k in range(len(rows))], bad=np.asarray(bad, np.uint8))


def _pair(arrays, mode, first, cand, frame):
    """(A, valid_a, B, valid_b) of one pair as the oracle takes them.  Mode 3: a frame feature whose valid byte is 0 is no candidate,
    which for the reference is a frame whose feature vector does not hold it."""
    bad = arrays["bad"]
    if mode == 4:
        A, B = arrays["kf"][first], arrays["kf"][cand]
        return A, good(A["row"], bad), B, good(B["row"], bad)
    A = arrays["kf"][cand]
    B = dict(frame)
    if frame.get("valid") is not None:   # the flat search and the oracle do not read the frame's valid: the filtered feature vector says the same
        B["bow"] = frame["bow"][frame["valid"][frame["bow"][:, 1]] != 0]
    return A, good(A["row"], bad), B, None


def reference(oracle, arrays, mode, cands, ratio, check_orientation, first=None, frame=None):
    """The oracle per pair.  mode 4: first = the first keyframe's slot; mode 3: frame = dict(kps, desc, valid or None, bow).  Returns
    dict(matched [n_pairs, n_out], matched_point, n_matches) as the batched call lays them out."""
    n_out = len(arrays["kf"][first]["kps"]) if mode == 4 else len(frame["kps"])
    out = dict(matched=np.full((len(cands), n_out), -1, np.int32), matched_point=np.full((len(cands), n_out), -1, np.int32), n_matches=np.zeros(len(cands), np.int32))
    for i, c in enumerate(cands):
        A, va, B, vb = _pair(arrays, mode, first, c, frame)
        if not len(A["kps"]) or not len(B["kps"]):
            continue
        n, m = oracle.search_by_bow(mode, A["kps"], A["desc"], va, csr(A["bow"]), B["kps"], B["desc"], vb, csr(B["bow"]), ratio, check_orientation)
        row = (B if mode == 4 else A)["row"]
        out["matched"][i], out["n_matches"][i] = m, n
        out["matched_point"][i] = np.where(m >= 0, row[np.maximum(m, 0)], -1)
        assert n == int((m >= 0).sum())
    return out


def assert_same(got, want, mode):
    key = "matched_second" if mode == 4 else "matched_kf_feature"
    assert np.array_equal(got["n_matches"], want["n_matches"]), (got["n_matches"], want["n_matches"])
    assert np.array_equal(got[key], want["matched"])
    assert np.array_equal(got["matched_point"], want["matched_point"])


def _distances(da, db):
    bits_a, bits_b = np.unpackbits(da, axis=1).astype(np.int16), np.unpackbits(db, axis=1).astype(np.int16)
    return bits_a @ (1 - bits_b).T + (1 - bits_a) @ bits_b.T


def analyse(arrays, mode, cand, ratio, first=None, frame=None):
    """One pair by brute force, orientation check off.  Returns dict(matched [n_out], n_matches, ratio_only = queries whose best passed
    the distance bound and failed the ratio test, taken = queries whose best valid candidate had gone to an earlier query, emptied =
    queries with a common node whose row entry is >= 0 but names a bad or never-set point, dropped = candidates left out for the same
    reason, records = the candidate records a gather writes, reserved = the pool entries it asks for (a query reserves its whole bucket
    before it knows which members are valid), common = nodes the two sides share)."""
    bad = arrays["bad"]
    A, va, B, vb = _pair(arrays, mode, first, cand, frame)
    vb = np.ones(len(B["kps"]), np.uint8) if vb is None else vb
    D = _distances(A["desc"], B["desc"])
    bucket = {}
    for node, feat in B["bow"]:
        bucket.setdefault(int(node), []).append(int(feat))
    taken_b = np.zeros(len(B["kps"]), bool)
    n_out = len(B["kps"]) if mode == 3 else len(A["kps"])
    r = dict(matched=np.full(n_out, -1, np.int32), n_matches=0, ratio_only=0, taken=0, emptied=0, dropped=0, records=0, reserved=0, common=set())
    b_row = B.get("row")
    for node, ia in A["bow"]:
        cands = bucket.get(int(node))
        if cands is None:
            continue
        r["common"].add(int(node))
        if not va[ia]:
            r["emptied"] += int(A["row"][ia] >= 0)
            continue
        valid = [c for c in cands if vb[c]]
        r["records"] += len(valid)
        r["reserved"] += len(cands)
        if b_row is not None:
            r["dropped"] += sum(1 for c in cands if b_row[c] >= 0 and not vb[c])
        free = [c for c in valid if not taken_b[c]]
        if not free:
            r["taken"] += int(len(valid) > 0)
            continue
        d = np.array([D[ia, c] for c in free])
        order = np.argsort(d, kind="stable")
        best, second = int(d[order[0]]), int(d[order[1]]) if len(free) > 1 else 256
        d_all = np.array([D[ia, c] for c in valid])
        if valid[int(np.argmin(d_all))] != free[int(order[0])]:
            r["taken"] += 1
        if best <= 50 and f32(best) < f32(ratio) * f32(second):
            c = free[int(order[0])]
            taken_b[c] = True
            r["matched"][c if mode == 3 else ia] = ia if mode == 3 else c
            r["n_matches"] += 1
        elif best <= 50:
            r["ratio_only"] += 1
    return r


_DEFAULT = None


def default_scene():
    """The default scene, built once: 300 base features, 4 candidates of 307 .. 328 features, a frame of 303, 12 vocabulary nodes."""
    global _DEFAULT
    if _DEFAULT is None:
        _DEFAULT = Scene()
    return _DEFAULT


SCENES = {
    "default": lambda: default_scene(),
    "buckets": lambda: Scene(seed=22, nodes=bucket_nodes, n_cand=2, twins=0, mapped=0.55),   # a twin would move a feature to another bucket
    "ends": lambda: Scene(seed=23, nodes=end_nodes, n_cand=2),
    "six_hundred": lambda: Scene(seed=24, n=600, n_cand=2, nodes=wide_nodes),
    "disjoint": lambda: Scene(seed=25, n_cand=3, disjoint=(2,)),
    "one_node": lambda: Scene(seed=26, n_cand=2, nodes=one_node),
}
_BUILT = {}


def scene(name):
    if name not in _BUILT:
        _BUILT[name] = SCENES[name]()
    return _BUILT[name]
