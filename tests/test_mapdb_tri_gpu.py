"""The resident table's BoW feature vectors and ydorb_mapdb_create_new_points on the GPU (ydorbslam_amd/csrc/map_resident.hip,
mapdb_tri_kernels.hip.h, orb_matcher.hip): the seeded sequence of tests/cpu_harness/mapdb_bow_check.cpp replayed through the real handle
against the naive model and that program's counters, and the query against the sequential CPU reference of tests/mapdb_tri_support.py
(the matcher oracle's search_for_triangulation composed with the CPU restatement of the geometry, claims carried between neighbours).
All five outputs are compared exactly, positions by bit pattern.  At most 600 features per keyframe and 5 neighbours."""
import numpy as np
import pytest

import mapdb_tri_support as T

pytestmark = pytest.mark.gpu
f32 = np.float32


def _db(bow=True, features=True, caps=(256, 16, 1024)):
    from ydorbslam_amd import MapDb
    db = MapDb(0, *caps)
    if features:
        db.enable_features()
    if bow:
        db.enable_bow()
    return db


def _run(scene, oracle, matcher=None, db=None, order=None, **flags):
    """Loads the scene into a fresh handle (or uses `db`), makes the call and holds it to the reference.  Returns (result, reference)."""
    import ydorbslam_amd as y
    own_db, own_m = db is None, matcher is None
    if own_db:
        db = _db()
        scene.load(db)
    if own_m:
        matcher = y.OrbMatcher(0.6, False)
    first, nbs, _keep = scene.call(order)
    got = db.create_new_points(matcher, first, nbs, **flags)
    want = scene.reference(oracle, order, **flags)
    assert not got["neighbour_status"].any()
    T.assert_same(got, want)
    if own_m:
        matcher.close()
    if own_db:
        db.close()
    return got, want


# ------------------------------------------------------------------------------------------------------------ the relation
def _all_stats(db):
    return db.stats(), db.row_stats(), db.desc_stats(), db.attr_stats(), db.feat_stats()


def test_the_seeded_sequence_equals_the_model_and_the_counters(tmp_path):
    ops = T.sequence(str(tmp_path))
    caps = (64, 16, 256)                                                        # the harness' kKeyframes
    db, plain = _db(caps=caps, features=False), _db(caps=caps, bow=False, features=False)
    n_kf = 1 + max(max(op[1]) for op in ops if op[0] == "set")
    assert n_kf > 16 and sum(op[0] == "sync" for op in ops) == 44 and sum(op[0] == "clear" for op in ops) == 1
    model = [np.zeros((0, 2), np.int64) for _ in range(n_kf)]
    for h in (db, plain):
        h.set_centres(np.arange(n_kf), np.zeros((n_kf, 3), f32))
    for op in ops:
        if op[0] == "set":
            db.set_keyframe_bow(op[1], op[2])
            for k, b in zip(op[1], op[2]):                                      # one after the other: the last value of a repeated slot wins
                model[k] = b
        elif op[0] == "clear":
            for h in (db, plain):
                h.clear()
                h.set_centres(np.arange(n_kf), np.zeros((n_kf, 3), f32))
            model = [np.zeros((0, 2), np.int64) for _ in range(n_kf)]
        else:
            trace = op[1]
            got = db.export_bow()
            assert len(got) == n_kf
            for k in range(n_kf):
                assert np.array_equal(got[k], model[k]), (trace["round"], k)
            s = db.bow_stats()
            assert s["enabled"] == 1 and {k: s[k] for k in trace if k != "round"} == {k: v for k, v in trace.items() if k != "round"}, trace["round"]
            plain.export()
            assert _all_stats(db) == _all_stats(plain)                          # every other stats struct keeps its values
    s = db.bow_stats()
    assert s["repacks_kept"] >= 1 and s["repacks_grown"] >= 2
    assert plain.bow_stats() == dict(enabled=0, repacks_kept=0, repacks_grown=0, n_entries=0, pool_used=0, pool_capacity=1, last_bow_sync_bytes=0,
                                     last_bow_sync_records=0)
    db.close()
    plain.close()


def test_a_handle_without_the_relation_refuses_the_new_entries(oracle_lib):
    import ydorbslam_amd as y
    s = T.default_scene()
    m = y.OrbMatcher(0.6, False)
    first, nbs, _keep = s.call()
    for bow, features, text in ((False, True, "keyframe BoW feature vectors are not enabled"), (True, False, "keyframe features are not enabled")):
        db = _db(bow=bow, features=features)
        db.set_centres(np.arange(8), np.zeros((8, 3), f32))
        with pytest.raises(y.YdorbError, match=text):
            db.create_new_points(m, first, nbs)
        if not bow:
            for call in (lambda: db.set_keyframe_bow([0], [s.kfs[0]["bow"]]), db.export_bow):
                with pytest.raises(y.YdorbError, match="keyframe BoW feature vectors are not enabled"):
                    call()
            assert db.bow_stats()["enabled"] == 0
        db.close()
    m.close()


def test_every_refusal_of_the_relation_reaches_the_caller():
    """The host check has each message; here: the C entry returns it, stages nothing, and enabling twice is fine."""
    import ydorbslam_amd as y
    db = _db(features=False)
    db.enable_bow()
    db.set_keyframe_bow([1], [[[3, 0], [3, 2], [9, 1]]])
    for bows, text in (([[[5, 0], [4, 1]]], "node id 4 after 5"), ([[[2 ** 31, 0]]], "node id 2147483648 outside"), ([[[1, 65535]]], "feature index 65535 outside"),
                       ([[[1, -1]]], "feature index -1 outside"), ([[[1, 7], [2, 7]]], "feature index 7 repeats inside its span"),
                       ([np.stack([np.arange(65536) // 9, np.arange(65536) % 65535], axis=1)], "a span of 65536 entries")):
        with pytest.raises(y.YdorbError, match=text):
            db.set_keyframe_bow([1], bows)
    with pytest.raises(y.YdorbError, match="negative keyframe slot -2"):
        db.set_keyframe_bow([-2], [[[1, 0]]])
    got = db.export_bow()
    assert np.array_equal(got[1], [[3, 0], [3, 2], [9, 1]]) and len(got[0]) == 0 and db.bow_stats()["n_entries"] == 3
    db.close()


# ------------------------------------------------------------------------------------------------------------ the query
def test_the_default_scene(oracle_lib):
    got, want = _run(T.default_scene(), oracle_lib)
    assert (got["n_matches"] >= 20).all() and (got["n_accepted"] >= 5).all()


def test_the_claims_decide_the_later_neighbours(oracle_lib):
    """Without the claim of an accepted idx1 (the geometry kernel's zeroing of the later neighbours' record counts) the call would give
    the reference computed without claims, which differs: the call equals the one and not the other."""
    import ydorbslam_amd as y
    s = T.default_scene()
    got, _ = _run(s, oracle_lib)
    without = s.reference(oracle_lib, claims=False)
    assert np.array_equal(got["matched_second"][0], without["matched_second"][0])
    assert any(not np.array_equal(got["matched_second"][i], without["matched_second"][i]) for i in range(1, s.n_nb))
    claimed = np.zeros(s.n, bool)
    for i in range(s.n_nb):                                                     # stated on the result alone: no accepted idx1 is ever matched again
        assert not (claimed & (got["matched_second"][i] >= 0)).any()
        claimed |= (got["status"][i] & 15) == 0


@pytest.mark.parametrize("flags", [dict(stereo_only=True), dict(check_orientation=True)], ids=["stereo_only", "check_orientation"])
def test_stereo_only_and_check_orientation(oracle_lib, flags):
    _run(T.default_scene(), oracle_lib, **flags)


def test_one_neighbour_alone_equals_the_flat_search_and_triangulation():
    """On the handle's own exports: Matcher.search_for_triangulation + triangulate_matches, the two flat calls the batched one replaces."""
    import ydorbslam_amd as y
    from ydorbslam_amd.triangulate import triangulate_matches
    s = T.default_scene()
    db, m = _db(), y.OrbMatcher(0.6, False)
    s.load(db)
    first, nbs, _keep = s.call([2])
    got = db.create_new_points(m, first, nbs)
    feats, blocks, rows, bows = db.export_features(), db.export_descriptors(), db.export_rows(), db.export_bow()
    a, b = s.slots[0], s.slots[2]

    def fv(bow):
        ids, counts = np.unique(bow[:, 0], return_counts=True)
        assert np.array_equal(np.repeat(ids, counts), bow[:, 0])
        return y.FeatureVector(ids, np.concatenate([[0], np.cumsum(counts)]), bow[:, 1])
    v1, v2 = dict(s.kfs[0]["view"]), dict(s.kfs[2]["view"])
    v1["kps"], v1["right_x"], v2["kps"], v2["right_x"] = feats[a][0], feats[a][1], feats[b][0], feats[b][1]
    n_m, match = m.search_for_triangulation(feats[a][0], blocks[a], (rows[a] >= 0).astype(np.uint8), feats[a][1], fv(bows[a]), feats[b][0], blocks[b],
                                            (rows[b] >= 0).astype(np.uint8), feats[b][1], fv(bows[b]), T.f12(v1, v2), T.epipole(v1, v2), v2["scale_factors"],
                                            v2["level_sigma2"])
    i1 = np.flatnonzero(match >= 0).astype(np.int32)
    r = triangulate_matches([v1, v2], [dict(first=0, second=1, idx1=i1, idx2=match[i1])])[0]
    assert n_m == got["n_matches"][0] >= 20 and np.array_equal(got["matched_second"][0], match)
    assert np.array_equal(got["status"][0, i1], r["status"]) and np.array_equal(got["x3d"][0, i1].view(np.uint32), r["x3d"].view(np.uint32))
    assert (got["status"][0, match < 0] == T.UNMATCHED).all() and not got["x3d"][0, match < 0].any() and got["n_accepted"][0] == r["n_accepted"]
    m.close()
    db.close()


def test_buckets_of_130_64_and_65_features(oracle_lib):
    _run(T.Scene(seed=6, nodes=T.bucket_nodes), oracle_lib)


def test_a_first_span_of_600_entries_stages_two_resolve_windows(oracle_lib):
    s = T.Scene(seed=9, n=600, n_nb=3)
    assert len(s.kfs[0]["bow"]) == 600
    got, _ = _run(s, oracle_lib)
    q = {int(f): i for i, f in enumerate(s.kfs[0]["bow"][:, 1])}                # the query behind each feature of the first keyframe
    matched_q = [q[int(i)] for i in np.flatnonzero(got["matched_second"][0] >= 0)]
    assert min(matched_q) < 512 <= max(matched_q)                               # matches on both sides of k_resolve's window of 512 queries


def test_nodes_below_and_above_the_second_span(oracle_lib):
    _run(T.Scene(seed=7, nodes=T.end_nodes), oracle_lib)


def test_a_neighbour_with_no_common_node_between_two_that_have_some(oracle_lib):
    s = T.Scene(seed=10, n_nb=3, disjoint=(2,))
    got, _ = _run(s, oracle_lib)
    assert got["n_matches"][1] == 0 and (got["matched_second"][1] == -1).all() and got["n_matches"][0] >= 20 and got["n_matches"][2] >= 20


def _untouched(got, i, n):
    return (got["matched_second"][i] == -1).all() and (got["status"][i] == T.UNMATCHED).all() and not got["x3d"][i].any() and got["n_matches"][i] == 0 and \
        got["n_accepted"][i] == 0


def test_every_neighbour_status_and_the_first_keyframe_unusable(oracle_lib):
    import ydorbslam_amd as y
    s = T.Scene(seed=11, n=120, n_nb=5)
    m = y.OrbMatcher(0.6, False)
    db = _db()
    s.load(db)
    sl, k = s.slots, s.kfs
    db.set_keyframe_features([sl[1]], [np.zeros(0, k[1]["view"]["kps"].dtype)], [np.zeros(0, f32)])      # neighbour 0: no feature span
    db.set_keyframe_descriptors([sl[2]], [np.zeros((0, 32), np.uint8)])                                  # neighbour 1: no descriptor block
    db.set_keyframe_bow([sl[3]], [np.zeros((0, 2), np.int64)])                                           # neighbour 2: no BoW span
    db.set_keyframe_rows([sl[4]], [k[4]["row"][:-1]])                                                    # neighbour 3: a row one short
    first, nbs, _keep = s.call()
    got = db.create_new_points(m, first, nbs)
    assert got["neighbour_status"].tolist() == [T.NB_STATUS[x] for x in ("no_features", "no_block", "no_bow", "length_mismatch", "ok")]
    assert all(_untouched(got, i, s.n) for i in range(4))
    want = s.reference(oracle_lib, order=[5])                                                            # the usable one is searched as if alone
    for key in want:
        assert np.array_equal(got[key][4:5].view(np.uint8), want[key].view(np.uint8)), key
    assert got["n_matches"][4] >= 10
    # the other length mismatches and the BoW index
    db.set_keyframe_rows([sl[4]], [k[4]["row"]])
    db.set_keyframe_descriptors([sl[4]], [k[4]["desc"][:-2]])
    bad = k[5]["bow"].copy()
    bad[-1, 1] = len(k[5]["row"])                                                                        # one past the last feature
    db.set_keyframe_bow([sl[5]], [bad])
    got = db.create_new_points(m, first, nbs)
    assert got["neighbour_status"][3:].tolist() == [T.NB_STATUS["length_mismatch"], T.NB_STATUS["bow_index"]] and _untouched(got, 3, s.n) and _untouched(got, 4, s.n)
    db.set_keyframe_descriptors([sl[4]], [k[4]["desc"]])
    db.set_keyframe_bow([sl[5]], [k[5]["bow"]])
    first2, nbs2, _keep2 = s.call()
    nbs2[3].view.n -= 1                                                                                  # a depth array one short
    got = db.create_new_points(m, first2, nbs2)
    assert got["neighbour_status"][3:].tolist() == [T.NB_STATUS["length_mismatch"], 0]
    # the first keyframe unusable: every neighbour has its status; an empty first span is "no BoW span"
    for stage, status in ((lambda: db.set_keyframe_bow([sl[0]], [np.zeros((0, 2), np.int64)]), "no_bow"),
                          (lambda: db.set_keyframe_descriptors([sl[0]], [np.zeros((0, 32), np.uint8)]), "no_block")):
        stage()
        got = db.create_new_points(m, first, nbs)
        assert (got["neighbour_status"] == T.NB_STATUS[status]).all() and all(_untouched(got, i, s.n) for i in range(5)), status
    m.close()
    db.close()


def test_a_pool_too_small_on_the_first_attempt_is_replayed_with_the_claims_reset(oracle_lib):
    """One vocabulary node: every eligible feature meets every feature of the neighbour, more records than a fresh matcher's pool holds
    per neighbour.  The attempt that overflows has searched only some queries and claimed from them; only a complete replay whose
    claims start afresh equals the reference."""
    import ydorbslam_amd as y
    s = T.Scene(seed=8, n_nb=2, nodes=T.one_node)
    m = y.OrbMatcher(0.6, False)                                                # fresh: its pool is at the initial size
    got, _ = _run(s, oracle_lib, matcher=m)
    assert (got["n_matches"] >= 20).all()
    _run(s, oracle_lib, matcher=m)                                              # and again on the grown pool, with no replay
    m.close()


def test_staged_row_feature_and_bow_deltas_pending_at_the_call(oracle_lib):
    """The call applies what is staged first: the table is loaded with another scene's keyframes and synced, then this scene's rows,
    features, blocks and feature vectors are staged and nothing is exported before the call."""
    other, s = T.Scene(seed=12, n=150, n_nb=3), T.Scene(seed=13, n=150, n_nb=3)
    s.slots = other.slots
    db = _db()
    other.load(db)
    db.export_bow()
    s.load(db)
    assert db.bow_stats()["last_bow_sync_records"] == 4                         # the export's sync; what was just staged is pending
    _run(s, oracle_lib, db=db)
    assert db.bow_stats()["last_bow_sync_records"] == 4 and db.feat_stats()["last_feat_sync_records"] == 4 and db.row_stats()["last_row_sync_records"] == 4
    # a single row entry staged: the feature gets a map point and is not matched any more
    got, _ = _run(s, oracle_lib, db=db)
    i1 = int(np.flatnonzero(got["matched_second"][0] >= 0)[0])
    db.set_row_entries([s.slots[0]], [i1], [3])
    s.kfs[0]["row"][i1] = 3
    got, _ = _run(s, oracle_lib, db=db)
    assert (got["matched_second"][:, i1] == -1).all()
    db.close()


def test_a_bow_pool_repack_and_a_feature_pool_repack_between_two_calls(oracle_lib):
    s = T.Scene(seed=14, n=150, n_nb=3)
    db = _db()
    s.load(db)
    _run(s, oracle_lib, db=db)
    before_b, before_f = db.bow_stats(), db.feat_stats()
    # other keyframes come and go until both pools have repacked: the scene's spans move
    spare = [k for k in range(12) if k not in s.slots][:3]
    for round_ in range(4):
        db.set_keyframe_bow(spare, [s.kfs[1 + (round_ + j) % 3]["bow"] for j in range(3)])
        db.set_keyframe_features(spare, [s.kfs[1 + (round_ + j) % 3]["view"]["kps"] for j in range(3)])
        db.export_bow()
    after_b, after_f = db.bow_stats(), db.feat_stats()
    assert after_b["repacks_kept"] + after_b["repacks_grown"] > before_b["repacks_kept"] + before_b["repacks_grown"]
    assert after_f["repacks_kept"] + after_f["repacks_grown"] > before_f["repacks_kept"] + before_f["repacks_grown"]
    _run(s, oracle_lib, db=db)
    db.close()


def test_no_neighbour_launches_nothing_and_writes_nothing():
    import ydorbslam_amd as y
    s = T.default_scene()
    db, m = _db(), y.OrbMatcher(0.6, False)
    s.load(db)
    first, _, _keep = s.call([])
    got = db.create_new_points(m, first, [])
    assert all(len(v) == 0 for v in got.values())
    assert db.bow_stats()["pool_used"] == 0                                     # not even the sync ran
    m.close()
    db.close()


def test_refused_up_front(oracle_lib):
    import ctypes as C
    import ydorbslam_amd as y
    s = T.default_scene()
    db, m = _db(), y.OrbMatcher(0.6, False)
    s.load(db)

    def call(change_first=None, change_nbs=None):
        first, nbs, _keep = s.call()
        if change_first:
            change_first(first)
        if change_nbs:
            change_nbs(nbs)
        return db.create_new_points(m, first, nbs)

    def setter(path, value):
        def f(obj):
            for name in path[:-1]:
                obj = getattr(obj, name) if isinstance(name, str) else obj[name]
            setattr(obj, path[-1], value)
        return f
    n_kf = db.n_keyframes
    for first_change, nb_change, text in ((setter(("n_levels",), 0), None, "first keyframe: n_levels 0 outside 1..8"),
                                          (setter(("n_levels",), 9), None, "first keyframe: n_levels 9 outside 1..8"),
                                          (None, setter((1, "view", "n_levels"), 9), "neighbour 1: n_levels 9 outside 1..8"),
                                          (setter(("kf_slot",), n_kf), None, "keyframe slot %d outside" % n_kf),
                                          (None, setter((2, "view", "kf_slot"), -1), "keyframe slot -1 outside"),
                                          (setter(("n",), s.n - 1), None, "the first keyframe has %d resident features, n is %d" % (s.n, s.n - 1)),
                                          (None, setter((1, "view", "kf_slot"), s.slots[0]), "neighbour 1 is the first keyframe"),
                                          (None, setter((3, "view", "kf_slot"), s.slots[2]), "neighbours 1 and 3 name keyframe slot %d twice" % s.slots[2]),
                                          (setter(("depth",), None), None, "first keyframe: negative n or null depth"),
                                          (None, setter((0, "view", "depth"), None), "neighbour 0: negative n or null depth")):
        with pytest.raises(y.YdorbError, match=text):
            call(first_change, nb_change)
    first, nbs, _keep = s.call()
    L = y.lib()
    nb = (type(nbs[0]) * len(nbs))(*nbs)
    out = np.zeros(s.n_nb * s.n * 3, f32)
    p = out.ctypes.data_as(C.c_void_p)
    for args, text in (((None, m._h, C.byref(first), nb, 4, 0, 0, p, p, p, p, p, p), "null handle"), ((db._h, None, C.byref(first), nb, 4, 0, 0, p, p, p, p, p, p), "null handle"),
                       ((db._h, m._h, None, nb, 4, 0, 0, p, p, p, p, p, p), "null first keyframe"), ((db._h, m._h, C.byref(first), None, 4, 0, 0, p, p, p, p, p, p), "null neighbours"),
                       ((db._h, m._h, C.byref(first), nb, 4, 0, 0, None, p, p, p, p, p), "null neighbours, matched_second"),
                       ((db._h, m._h, C.byref(first), nb, 4, 0, 0, p, p, p, p, p, None), "null neighbours, matched_second"),
                       ((db._h, m._h, C.byref(first), nb, -1, 0, 0, p, p, p, p, p, p), "negative number of neighbours")):
        assert L.ydorb_mapdb_create_new_points(*args) == -1 and text.encode() in L.ydorb_last_error(), text
    _run(s, oracle_lib, db=db, matcher=m)                                       # the refused calls left the table and the matcher as they were
    m.close()
    db.close()
