"""The resident table's keyframe features and ydorb_mapdb_fuse_search on the GPU (ydorbslam_amd/csrc/map_resident.hip,
mapdb_feat_kernels.hip.h, mapdb_fuse_kernels.hip.h, orb_matcher.hip): the seeded sequence of tests/cpu_harness/mapdb_feat_check.cpp
replayed through the real handle against the naive model and that program's counters, and the batched search against (a) the CPU
restatement of pass 1 (tests/fuse_ref) composed with the oracle's fuse_search, used unchanged, and (b) the flat path: the restatement's
queries and descriptors pushed through ydorb_window_search per target, on keyframes gathered from the handle's exports.  Every
comparison is exact.  At most 600 points, 16 keyframes and 400 features per keyframe."""
import numpy as np
import pytest

import mapdb_fuse_support as R

pytestmark = pytest.mark.gpu
I32 = np.int32
f32 = np.float32


def _db(caps=(1024, 16, 8192), features=True, attributes=True):
    from ydorbslam_amd import MapDb
    db = MapDb(0, *caps)
    if attributes:
        db.enable_attributes()
    if features:
        db.enable_features()
    return db


def _all_stats(db):
    return db.stats(), db.row_stats(), db.desc_stats(), db.attr_stats()


# ------------------------------------------------------------------------------------------------------------ the relation
def test_the_seeded_sequence_equals_the_model_and_the_counters(tmp_path):
    rounds = R.sequence(str(tmp_path))
    assert len(rounds) == 40
    caps = (64, R.SEQUENCE_KEYFRAMES, 256)
    db, plain = _db(caps, attributes=False), _db(caps, features=False, attributes=False)
    n_kf = 1 + max(int(op[1].max()) for ops in rounds for op in ops if op[0] == "F")
    assert n_kf > R.SEQUENCE_KEYFRAMES                                          # the headers grow on the way
    for h in (db, plain):                                                       # both hold every keyframe slot from the start
        h.set_centres(np.arange(n_kf), np.zeros((n_kf, 3), f32))
    model = [np.zeros(0, R.rec_dtype()) for _ in range(n_kf)]
    for ops in rounds:
        for op in ops:
            if op[0] == "F":
                _, kfs, stereo, recs = op
                db.set_keyframe_features(kfs, [r["kp"] for r in recs], [r["right_x"] for r in recs] if stereo else None)
                for k, r in zip(kfs, recs):                                     # one after the other: the last value of a repeated slot wins
                    model[k] = r
            else:
                trace = op[1]
                got = db.export_features()
                assert len(got) == n_kf
                for k in range(n_kf):
                    assert got[k][0].tobytes() == model[k]["kp"].tobytes() and got[k][1].tobytes() == model[k]["right_x"].tobytes(), (trace["round"], k)
                s = db.feat_stats()
                assert s["enabled"] == 1 and {k: s[k] for k in R.TRACE_FIELDS[1:]} == {k: trace[k] for k in R.TRACE_FIELDS[1:]}, trace["round"]
                plain.export()
                assert _all_stats(db) == _all_stats(plain)                      # the other four stats structs do not move
    s = db.feat_stats()
    assert s["repacks_kept"] >= 1 and s["repacks_grown"] >= 2
    assert plain.feat_stats() == dict(enabled=0, repacks_kept=0, repacks_grown=0, n_features=0, pool_used=0, pool_capacity=1, last_feat_sync_bytes=0,
                                      last_feat_sync_records=0)
    db.clear()
    after = db.feat_stats()
    assert after["n_features"] == 0 and after["pool_used"] == 0 and after["pool_capacity"] == s["pool_capacity"] and after["repacks_grown"] == s["repacks_grown"]
    db.set_centres(np.arange(n_kf), np.zeros((n_kf, 3), f32))
    assert all(len(k) == 0 for k, _ in db.export_features())
    db.set_keyframe_features([2], [model[0]["kp"]], [model[0]["right_x"]])      # clear, then reuse
    assert db.export_features()[2][0].tobytes() == model[0]["kp"].tobytes()
    db.close()
    plain.close()


def test_a_handle_without_the_relation_refuses_the_new_entries():
    import ydorbslam_amd as y
    s = R.Scene(n_kf=2, n_feat=20, n_points=30)
    m = y.OrbMatcher(0.6, True)
    for attributes, features, text in ((True, False, "keyframe features are not enabled"), (False, True, "point attributes are not enabled")):
        db = _db(attributes=attributes, features=features)
        db.set_centres([0, 1], np.zeros((2, 3), f32))
        with pytest.raises(y.YdorbError, match=text):
            db.fuse_search(m, [s.target(0)], [[0]], [[0]])
        if not features:
            for call in (lambda: db.set_keyframe_features([0], [s.kps[0]]), db.export_features):
                with pytest.raises(y.YdorbError, match="keyframe features are not enabled"):
                    call()
            assert db.feat_stats()["enabled"] == 0
        db.close()


# ------------------------------------------------------------------------------------------------------------ the query
def _check(db, matcher, targets, lists, skips, want_target_status=None, probe=None):
    """One batched call against the restatement + oracle and against the flat path, on the handle's own exports (read after the call,
    so that what was staged at the call is applied by the call itself; probe() runs between the call and the exports).  Returns the call's result
    and the restatement's."""
    got = db.fuse_search(matcher, targets, lists, skips)
    if probe is not None:
        probe()
    m, feats, blocks = R.exported_map(db), db.export_features(), db.export_descriptors()
    ref = R.ref_queries(m, targets, lists, skips)
    assert len(got) == len(targets)
    for t, (G, g, r) in enumerate(zip(targets, got, ref)):
        kps, rx = feats[G.kf_slot]
        desc = blocks[G.kf_slot]
        want_ts = 1 if len(kps) == 0 else 2 if len(desc) == 0 else 3 if len(desc) != len(kps) else 0
        assert g["target_status"] == want_ts, t
        if want_target_status is not None:
            assert want_ts == want_target_status[t], t
        assert np.array_equal(g["status"], r["status"]), t
        if want_ts != 0:
            assert g["n_found"] == 0 and (g["best_idx"] == -1).all(), t
            continue
        n_ref, b_ref = R.oracle_search(kps, desc, rx, G, r)
        assert g["n_found"] == n_ref and np.array_equal(g["best_idx"], b_ref), t
        if len(r["queries"]):
            import ydorbslam_amd as y
            V = G.view
            fv = y.FrameView(kps, desc, (V.min_x, V.max_x, V.min_y, V.max_y), None if (G.flags & R.MONOCULAR) else rx)
            n_flat, b_flat = matcher.fuse_search(fv, r["queries"], r["qdesc"], np.array(G.inv_sigma2[:], f32), G.max_dist)
            assert g["n_found"] == n_flat and np.array_equal(g["best_idx"], b_flat), t
    return got, ref


@pytest.fixture(scope="module")
def world():
    import ydorbslam_amd as y
    s = R.Scene()
    db = _db()
    s.load(db)
    yield s, db, y.OrbMatcher(0.6, True)
    db.close()


def _all(s, rng, n=None):
    slots = rng.permutation(s.n_points).astype(I32) if n is None else rng.integers(0, s.n_points, n).astype(I32)
    return slots, (rng.uniform(size=len(slots)) < 0.05).astype(np.uint8)


def test_three_targets_with_an_empty_list_between_and_one_target(world):
    s, db, m = world
    rng = np.random.default_rng(1)
    a, b = _all(s, rng), _all(s, rng, 300)
    empty = (np.zeros(0, I32), np.zeros(0, np.uint8))
    got, ref = _check(db, m, [s.target(0), s.target(1), s.target(2)], [a[0], empty[0], b[0]], [a[1], empty[1], b[1]], [0, 0, 0])
    assert got[0]["n_found"] > 10 and got[2]["n_found"] > 5 and got[1]["n_found"] == 0
    seen = set(np.concatenate([r["status"] for r in ref]).tolist())
    assert seen == set(R.STATUS.values())
    got1, _ = _check(db, m, [s.target(0)], [a[0]], [a[1]])
    assert np.array_equal(got1[0]["best_idx"], got[0]["best_idx"])                 # a target's answer does not depend on its company
    before = db.feat_stats(), db.desc_stats(), db.attr_stats()
    db.fuse_search(m, [s.target(3)], [a[0]], [a[1]])
    now = db.feat_stats(), db.desc_stats(), db.attr_stats()
    assert now == before and now[0]["last_feat_sync_bytes"] == 0                   # with nothing staged no map byte moves


@pytest.mark.parametrize("length", [0, 1, 63, 64, 65, 257])
def test_list_lengths(world, length):
    s, db, m = world
    rng = np.random.default_rng(100 + length)
    good = np.flatnonzero((s.bad == 0) & (s.flags == 3))
    slots = rng.choice(good, length, replace=length > len(good)).astype(I32)
    got, _ = _check(db, m, [s.target(4)], [slots], [np.zeros(length, np.uint8)])
    assert len(got[0]["best_idx"]) == length
    if length >= 63:
        other = _all(s, rng, 70)
        _check(db, m, [s.target(5), s.target(4)], [other[0], slots], [other[1], np.zeros(length, np.uint8)])


def test_a_stereo_target_the_same_target_monocular_and_the_zero_sigma_table(world):
    s, db, m = world
    rng = np.random.default_rng(2)
    a = _all(s, rng)
    targets = [s.target(1), s.target(1, flags=R.SKIP_OBSERVED | R.MONOCULAR), s.target(1, flags=R.MONOCULAR, inv_sigma2=R.ZERO_SIGMA2, max_dist=100),
               s.target(1, flags=R.MONOCULAR, inv_sigma2=R.ZERO_SIGMA2)]
    got, _ = _check(db, m, targets, [a[0]] * 4, [a[1]] * 4)
    assert (s.right_x[1] >= 0).sum() > 20
    assert got[0]["n_found"] > 5 and got[1]["n_found"] > 5 and not np.array_equal(got[0]["best_idx"], got[1]["best_idx"])
    assert got[2]["n_found"] >= got[3]["n_found"] > 0 and got[2]["n_found"] > got[3]["n_found"]


def test_one_case_per_entry_status():
    """A point the target searches, then copies of it that differ in the one thing a rule reads."""
    import ydorbslam_amd as y
    s = R.Scene(seed=5, n_kf=3, n_feat=120, n_points=150)
    m = y.OrbMatcher(0.6, True)
    k = 0
    G = s.target(k)
    base = R.ref_queries(R.scene_map(s), [G], [np.arange(s.n_points)], [np.zeros(s.n_points, np.uint8)])[0]
    p = int(np.flatnonzero(base["status"] == 0)[0])
    Ow = s.poses[k][1].astype(np.float64)
    P = s.pos[p].astype(np.float64)
    dist = float(np.linalg.norm(P - Ow))
    Rcw = s.poses[k][0][:, :3].astype(np.float64)
    n0 = s.n_points
    side = P + Rcw.T @ np.array([dist * 3, 0, 0])
    cases = [("searched", dict()), ("skipped", dict()), ("bad", dict(bad=1)), ("observed", dict(observers=[2, k])),
             ("no_attributes", dict(flags=R.DESCRIPTOR)), ("no_attributes", dict(flags=R.GEOMETRY)),
             ("rejected", dict(pos=(Ow - (P - Ow)).astype(f32), normal=-s.normal[p])),          # zc < 0, everything else holds
             ("rejected", dict(pos=side.astype(f32), normal=((side - Ow) / np.linalg.norm(side - Ow)).astype(f32), mx=f32(dist * 8), mn=f32(0))),   # outside the image
             ("rejected", dict(mn=f32(dist * 2))),                                              # dist < 0.8 min
             ("rejected", dict(mx=f32(dist / 2), mn=f32(0))),                                   # dist > 1.2 max
             ("rejected", dict(normal=-s.normal[p])),                                           # the viewing angle
             ("rejected", dict(pos=np.array([np.nan, P[1], P[2]], f32)))]                       # NaN
    slots = [s.clone_point(p, **ch) for _, ch in cases]
    never = s.clone_point(p, gap=1) - 1                                                         # a slot never set counts as bad
    last = s.n_points - 1
    db = _db()
    db.enable_attributes()
    db.set_centres(np.arange(s.n_kf), np.stack([o for _, o in s.poses]))
    s.load_points(db, [q for q in range(s.n_points) if q != never])
    s.load_keyframes(db)
    listed = np.array(slots + [never, last], I32)
    skip = np.array([1 if name == "skipped" else 0 for name, _ in cases] + [0, 0], np.uint8)
    got, _ = _check(db, m, [G, s.target(k, flags=0)], [listed, listed], [skip, skip])
    want = [R.STATUS[name] for name, _ in cases] + [R.STATUS["bad"], R.STATUS["searched"]]
    assert got[0]["status"].tolist() == want and n0 + len(cases) + 2 == s.n_points
    want[3] = R.STATUS["searched"]                                                              # without flag bit 0 isInKeyFrame is not asked
    assert got[1]["status"].tolist() == want
    assert got[0]["best_idx"][0] == got[0]["best_idx"][-1] and (got[0]["best_idx"][1:-1] == -1).all()
    db.close()


def test_target_corner_cases():
    """Targets with 0 features, 1 feature, a missing block and a block of another length, beside a good one."""
    import ydorbslam_amd as y
    s = R.Scene(seed=6, n_kf=6, n_feat=80, n_points=120)
    m = y.OrbMatcher(0.6, True)
    db = _db()
    s.load(db)
    db.set_keyframe_features([1], [s.kps[1][:0]], [s.right_x[1][:0]])           # erased: no feature span
    db.set_keyframe_descriptors([2], [s.desc[2][:0]])                           # no block
    db.set_keyframe_descriptors([3], [s.desc[3][:50]])                          # the lengths differ
    db.set_keyframe_features([4], [s.kps[4][:1]], [s.right_x[4][:1]])           # one feature ...
    db.set_keyframe_descriptors([4], [s.desc[4][:1]])                           # ... and its descriptor
    rng = np.random.default_rng(3)
    lists, skips = zip(*[_all(s, rng) for _ in range(6)])
    got, _ = _check(db, m, [s.target(k) for k in (0, 1, 2, 3, 4, 5)], lists, skips, [0, 1, 2, 3, 0, 0])
    assert got[0]["n_found"] > 0 and got[5]["n_found"] > 0
    _check(db, m, [s.target(k) for k in (1, 2, 3)], lists[:3], skips[:3], [1, 2, 3])     # no target searches anything
    # one feature, and a point made to meet it
    j, T, Ow = 0, *s.poses[4]
    z, lvl = 4.0, int(s.kps[4]["octave"][0])
    uv = np.array([s.kps[4]["x"][j] - (R.SF[lvl] + 0.3), s.kps[4]["y"][j]], np.float64)
    Xc = np.array([(uv[0] - R.F.K[2]) * z / R.F.K[0], (uv[1] - R.F.K[3]) * z / R.F.K[1], z])
    P = T[:, :3].astype(np.float64).T @ (Xc - T[:, 3].astype(np.float64))
    d = float(np.linalg.norm(P - Ow))
    q = s.clone_point(0, pos=P.astype(f32), normal=((P - Ow) / d).astype(f32), mx=f32(d * 1.2 ** (lvl - 0.5)), mn=f32(0), pdesc=s.desc[4][0], bad=0, flags=3,
                      observers=[])
    s.load_points(db, [q])
    got, _ = _check(db, m, [s.target(4, flags=R.MONOCULAR)], [[q, q]], [[0, 0]], [0])
    assert got[0]["best_idx"].tolist() == [0, 0] and got[0]["n_found"] == 2    # a slot repeated in one list: nothing is taken, both match
    db.close()


def _crowd(n_feat, n_points, octave=2):
    """One keyframe whose n_feat features lie in a row 0.01 px apart around one spot, and n_points points that project beside the row so
    that every feature is a candidate of every point (x distance above r, same level): a window of n_feat records per query."""
    from ydorbslam_amd import KP_DTYPE
    s = R.Scene(seed=8, n_kf=2, n_feat=4, n_points=4)
    rng = np.random.default_rng(9)
    kp = np.zeros(n_feat, KP_DTYPE)
    kp["x"], kp["y"] = 300.0 + 0.01 * np.arange(n_feat), 200.0
    kp["octave"], kp["size"], kp["class_id"] = octave, 31, -1
    s.kps[0], s.right_x[0], s.desc[0] = kp, np.full(n_feat, -1.0, f32), rng.integers(0, 256, (n_feat, 32), dtype=np.uint8)
    T, Ow = s.poses[0]
    Rm, t = T[:, :3].astype(np.float64), T[:, 3].astype(np.float64)
    r = float(R.SF[octave])
    pts = []
    for i in range(n_points):
        z = rng.uniform(2.0, 6.0)
        uv = np.array([300.0 - r - 0.5 - rng.uniform(0, 0.5), 200.0 + rng.normal(0, 0.2)])
        Xc = np.array([(uv[0] - R.F.K[2]) * z / R.F.K[0], (uv[1] - R.F.K[3]) * z / R.F.K[1], z])
        P = Rm.T @ (Xc - t)
        d = float(np.linalg.norm(P - Ow))
        pts.append(s.clone_point(0, pos=P.astype(f32), normal=((P - Ow) / d).astype(f32), mx=f32(d * 1.2 ** (octave - 0.5)), mn=f32(0),
                                 pdesc=s.desc[0][int(rng.integers(0, n_feat))], bad=0, flags=3, observers=[]))
    return s, np.array(pts, I32)


def test_a_window_of_more_than_a_slot_uses_the_overflow_region_and_a_pool_too_small_is_replayed():
    """120 features inside every window: each query holds more than kSlot = 64 records, so they lie in the overflow region.  Then 400
    features and 100 points: 40 000 records of one call against an overflow region of 16 384 at first - the gather kernel reports the
    overflow, the entry grows the region to what the heads asked for and replays; only a complete replay equals the oracle, whose
    winners lie anywhere in the 400.  A second matcher handle starts small again and must agree."""
    import ydorbslam_amd as y
    for n_feat, n_points in ((120, 40), (400, 100)):
        s, pts = _crowd(n_feat, n_points)
        db = _db()
        s.load(db)
        for m in (y.OrbMatcher(0.6, True), y.OrbMatcher(0.6, True)):
            G = s.target(0, flags=R.MONOCULAR, inv_sigma2=R.ZERO_SIGMA2)
            got, ref = _check(db, m, [G, s.target(1)], [pts, pts[:10]], [np.zeros(len(pts), np.uint8), np.zeros(10, np.uint8)])
            assert (ref[0]["status"] == 0).all() and got[0]["n_found"] == n_points
            assert len(set(got[0]["best_idx"].tolist())) > 10
            _check(db, m, [G], [pts], [np.zeros(len(pts), np.uint8)])             # the grown pool serves the next call at once
        db.close()


def test_the_same_point_for_two_targets_and_staged_changes_at_the_call(world):
    s, db, m = world
    rng = np.random.default_rng(4)
    slots = rng.permutation(s.n_points)[:200].astype(I32)
    skip = np.zeros(200, np.uint8)
    got, _ = _check(db, m, [s.target(0), s.target(2)], [slots, slots], [skip, skip])
    assert got[0]["n_found"] > 0 and got[1]["n_found"] > 0
    # features, block and attributes of a keyframe and of points staged and not synced when the call is made
    s2 = R.Scene(seed=21, n_kf=s.n_kf, n_feat=150, n_points=s.n_points)
    s2.poses = s.poses
    s2.load_keyframes(db, [2])
    s2.load_points(db, np.arange(0, 100))
    assert db.feat_stats()["n_features"] != db.feat_stats()["pool_used"]       # staged, not applied
    def the_call_applied_them():
        assert db.feat_stats()["last_feat_sync_records"] == 1 and db.feat_stats()["n_features"] == db.feat_stats()["pool_used"] - 200
        assert 90 <= db.attr_stats()["last_attr_sync_records"] <= 100 and db.desc_stats()["last_desc_sync_records"] == 1

    _check(db, m, [s.target(2), s.target(0)], [slots, slots], [skip, skip], probe=the_call_applied_them)
    assert len(db.export_features()[2][0]) == 150
    s.load_keyframes(db, [2])                                                   # and back, for the tests that share the handle
    none = [np.zeros(0, I32)] * 100                                             # erased first: a group the first scene's point lacks must not stay
    db.set_points(np.arange(100), none, [np.zeros(0, np.uint8)] * 100, np.ones(100, np.uint8), np.zeros(100, I32), np.zeros(100, np.uint8), np.zeros((100, 3), f32))
    s.load_points(db, np.arange(0, 100))
    got3, _ = _check(db, m, [s.target(0), s.target(2)], [slots, slots], [skip, skip])
    assert all(np.array_equal(a["best_idx"], b["best_idx"]) for a, b in zip(got, got3))


def test_a_feature_pool_repack_and_a_point_table_growth_between_two_calls():
    import ydorbslam_amd as y
    s = R.Scene(seed=12, n_kf=5, n_feat=100, n_points=200)
    m = y.OrbMatcher(0.6, True)
    db = _db(caps=(256, 4, 1024))
    s.load(db)
    rng = np.random.default_rng(5)
    a = _all(s, rng)
    first, _ = _check(db, m, [s.target(1), s.target(3)], [a[0], a[0]], [a[1], a[1]])
    before = db.feat_stats(), db.stats()
    for _ in range(3):                                                          # keyframes re-staged until the pool must repack
        s.load_keyframes(db, [0, 2, 4])
        db.export_features()
    mid = db.feat_stats()
    assert mid["repacks_kept"] + mid["repacks_grown"] > before[0]["repacks_kept"] + before[0]["repacks_grown"]
    again, _ = _check(db, m, [s.target(1), s.target(3)], [a[0], a[0]], [a[1], a[1]])
    assert all(np.array_equal(x["best_idx"], y_["best_idx"]) and np.array_equal(x["status"], y_["status"]) for x, y_ in zip(first, again))
    extra = [s.clone_point(int(p)) for p in rng.integers(0, 200, 100)]          # the point table grows past its capacity of 256
    s.load_points(db, extra)
    b = np.concatenate([a[0], np.array(extra, I32)])
    grown, _ = _check(db, m, [s.target(1), s.target(3)], [b, b], [np.zeros(len(b), np.uint8)] * 2)
    assert db.stats()["point_table_growths"] > before[1]["point_table_growths"] and db.attr_stats()["growths"] >= 1
    assert grown[0]["n_found"] >= first[0]["n_found"]
    db.close()


def test_refused_up_front(world):
    import ydorbslam_amd as y
    s, db, m = world
    ok = ([s.target(0)], [[1, 2]], [[0, 0]])
    for change, text in ((lambda G: setattr(G, "kf_slot", s.n_kf), "keyframe slot %d outside" % s.n_kf), (lambda G: setattr(G, "kf_slot", -1), "keyframe slot -1 outside"),
                         (lambda G: setattr(G, "max_dist", 257), "max_dist 257 outside 0..256"), (lambda G: setattr(G, "max_dist", -1), "max_dist -1 outside"),
                         (lambda G: setattr(G.view, "n_levels", 9), "n_levels 9 outside 1..8"), (lambda G: setattr(G.view, "n_levels", 0), "n_levels 0 outside")):
        G = s.target(0)
        change(G)
        with pytest.raises(y.YdorbError, match=text):
            db.fuse_search(m, [G], ok[1], ok[2])
    with pytest.raises(y.YdorbError, match="point slot %d outside" % s.n_points):
        db.fuse_search(m, ok[0], [[1, s.n_points]], ok[2])
    with pytest.raises(y.YdorbError, match="point slot -1 outside"):
        db.fuse_search(m, ok[0], [[-1, 2]], ok[2])
    L = y.lib()
    one, bad_start = np.zeros(2, I32), np.array([1, 2], I32)
    p = R._p
    assert L.ydorb_mapdb_fuse_search(db._h, m._h, None, 1, p(one), p(one), p(one), p(one), p(one), p(one), p(one)) == -1 and b"null targets" in L.ydorb_last_error()
    assert L.ydorb_mapdb_fuse_search(db._h, m._h, None, 0, p(bad_start), None, None, None, None, None, None) == -1 and b"list_start[0] is 1" in L.ydorb_last_error()
    assert L.ydorb_mapdb_fuse_search(db._h, m._h, None, 0, None, None, None, None, None, None, None) == -1 and b"null list_start" in L.ydorb_last_error()
    assert db.fuse_search(m, [], [], []) == []                                  # nothing to do: OK and nothing launched
    got = db.fuse_search(m, [s.target(0), s.target(1)], [[], []], [[], []])
    assert [g["n_found"] for g in got] == [0, 0] and [g["target_status"] for g in got] == [0, 0]
