"""ydorb_mapdb_search_by_bow_keyframes / ydorb_mapdb_search_by_bow_frame on the GPU (ydorbslam_amd/csrc/mapdb_bow_kernels.hip.h,
orb_matcher.hip, map_resident.hip): every output of the batched calls against the matcher oracle's search_by_bow per pair, on arrays
gathered from the handle's own exports with "has a good map point" computed in Python (tests/mapdb_bowsearch_support.py).  All
comparisons are exact, for both forms, with check_orientation 0 and 1 and ratio 0.6, 0.75 and 0.9.  tests/test_mapdb_bowsearch_cpu.py
proves on the reference alone that the scenes can tell a wrong search from a right one.  At most 600 features per keyframe and 4
candidates."""
import ctypes as C

import numpy as np
import pytest

import mapdb_bowsearch_support as B

pytestmark = pytest.mark.gpu
f32 = np.float32
MODES = pytest.mark.parametrize("mode", [4, 3], ids=["keyframes", "frame"])


def _db(scene=None, caps=(1024, 16, 1024), skip=()):
    from ydorbslam_amd import MapDb
    db = MapDb(0, *caps)
    if scene is not None:
        scene.load(db, skip)
    return db


def _matcher():
    import ydorbslam_amd as y
    return y.OrbMatcher(0.6, False)


def _call(db, m, s, mode, cands, ratio=0.6, ori=False, valid=True):
    if mode == 4:
        r = db.search_by_bow_keyframes(m, s.slots[0], cands, len(s.kfs[0]["kps"]), ratio, ori)
        r["matched"] = r["matched_second"]
    else:
        r = db.search_by_bow_frame(m, cands, *s.frame_args(valid), ratio, ori)
        r["matched"] = r["matched_kf_feature"]
    return r


def _want(oracle, arrays, s, mode, cands, ratio=0.6, ori=False, valid=True):
    if mode == 4:
        return B.reference(oracle, arrays, 4, cands, ratio, ori, first=s.slots[0])
    frame = dict(s.frame) if valid else dict(s.frame, valid=None)
    return B.reference(oracle, arrays, 3, cands, ratio, ori, frame=frame)


def _check(db, m, s, oracle, mode, cands=None, arrays=None, every=True, valid=True, status=0):
    """The batched call against the reference for every ratio and both orientation settings (every=False: ratio 0.6, no check only)."""
    cands = s.slots[1:] if cands is None else cands
    arrays = B.gather(db) if arrays is None else arrays
    got = None
    for ratio in (B.RATIOS if every else B.RATIOS[:1]):
        for ori in ((False, True) if every else (False,)):
            got = _call(db, m, s, mode, cands, ratio, ori, valid)
            B.assert_same(got, _want(oracle, arrays, s, mode, cands, ratio, ori, valid), mode)
            assert (got["pair_status"] == status).all()
    return got


def _all_stats(db):
    return db.stats(), db.row_stats(), db.desc_stats(), db.attr_stats(), db.feat_stats(), db.bow_stats(), db.lba_stats()


# ------------------------------------------------------------------------------------------------------------ the scenes
@MODES
def test_the_default_scene_with_four_candidates(oracle_lib, mode):
    s = B.default_scene()
    db, m = _db(s), _matcher()
    got = _check(db, m, s, oracle_lib, mode)
    assert got["matched"].shape == (4, 300 if mode == 4 else 303) and got["matched_point"].shape == got["matched"].shape
    assert (got["n_matches"] >= 10).all()
    st = m.bow_search_stats()
    assert st["launches"] == 4 and st["synchronisations"] == 1 and st["attempts"] == st["calls"] == 6   # per call, whatever the number of pairs
    if mode == 3:
        _check(db, m, s, oracle_lib, mode, valid=False)                       # a null valid: every frame feature is a candidate
    m.close()
    db.close()


@MODES
def test_the_batched_call_equals_one_flat_search_per_candidate(mode):
    """On the handle's own exports: OrbMatcher.search_by_bow per pair, the flat call the batched one replaces (the flat frame form reads
    no valid bytes, so the frame goes without)."""
    import ydorbslam_amd as y
    s = B.default_scene()
    db = _db(s)
    arrays = B.gather(db)
    for ratio in B.RATIOS:
        for ori in (False, True):
            m = y.OrbMatcher(ratio, ori)
            got = _call(db, m, s, mode, s.slots[1:], ratio, ori, valid=False)
            for i, c in enumerate(s.slots[1:]):
                A = arrays["kf"][s.slots[0] if mode == 4 else c]
                Bs = arrays["kf"][c] if mode == 4 else s.frame
                n, out = m.search_by_bow(mode, A["kps"], A["desc"], B.good(A["row"], arrays["bad"]), y.FeatureVector(*B.csr(A["bow"])), Bs["kps"], Bs["desc"],
                                         B.good(Bs["row"], arrays["bad"]) if mode == 4 else None, y.FeatureVector(*B.csr(Bs["bow"])))
                assert n == got["n_matches"][i] and np.array_equal(out, got["matched"][i]), (ratio, ori, i)
            m.close()
    db.close()


@MODES
@pytest.mark.parametrize("name", ["buckets", "ends", "six_hundred", "disjoint"])
def test_the_other_scenes(oracle_lib, mode, name):
    s = B.scene(name)
    db, m = _db(s), _matcher()
    got = _check(db, m, s, oracle_lib, mode)
    if name == "disjoint":
        assert got["n_matches"][1] == 0 and (got["matched"][1] == -1).all() and (got["matched_point"][1] == -1).all()
    assert m.bow_search_stats()["pool_per_pair"] == B.POOL_PER_PAIR            # none of these needed the replay
    m.close()
    db.close()


@MODES
def test_a_pool_too_small_on_the_first_attempt_is_replayed(oracle_lib, mode):
    s = B.scene("one_node")
    db, m = _db(s), _matcher()                                               # a fresh matcher: its pool is at the initial size
    arrays = B.gather(db)
    got = _check(db, m, s, oracle_lib, mode, arrays=arrays, every=False)
    st = m.bow_search_stats()
    assert st["calls"] == 1 and st["attempts"] == 2 and st["launches"] == 8 and st["synchronisations"] == 2 and st["pool_per_pair"] > B.POOL_PER_PAIR
    assert (got["n_matches"] >= 30).all()
    _check(db, m, s, oracle_lib, mode, arrays=arrays)                         # and again on the grown pool, with no replay
    st2 = m.bow_search_stats()
    assert st2["attempts"] - st["attempts"] == st2["calls"] - st["calls"] == 6 and st2["pool_per_pair"] == st["pool_per_pair"]
    m.close()
    db.close()


# ------------------------------------------------------------------------------------------------------------ the candidate list
@MODES
def test_repeats_the_first_keyframe_as_a_candidate_one_candidate_and_none(oracle_lib, mode):
    s = B.default_scene()
    db, m = _db(s), _matcher()
    arrays = B.gather(db)
    c = s.slots[1:]
    got = _check(db, m, s, oracle_lib, mode, cands=[c[1], c[0], c[1], s.slots[0], c[1]], arrays=arrays)
    for key in ("matched", "matched_point", "n_matches"):
        assert np.array_equal(got[key][0], got[key][2]) and np.array_equal(got[key][0], got[key][4])   # repeats answer alike
    assert got["n_matches"][3] >= 30                                          # a keyframe against itself
    one = _check(db, m, s, oracle_lib, mode, cands=[c[2]], arrays=arrays)
    assert one["matched"].shape[0] == 1
    before, stats = m.bow_search_stats(), _all_stats(db)
    db.set_row_entries([s.slots[0]], [0], [-1])                               # something staged: an empty call must not apply it
    none = _call(db, m, s, mode, [])
    assert all(len(none[k]) == 0 for k in ("matched", "matched_point", "n_matches", "pair_status"))
    assert m.bow_search_stats() == before and db.row_stats()["last_row_sync_records"] == stats[1]["last_row_sync_records"]
    m.close()
    db.close()


def test_a_frame_without_features_and_a_frame_without_nodes(oracle_lib):
    import ydorbslam_amd as y
    s = B.default_scene()
    db, m = _db(s), _matcher()
    empty = y.FeatureVector(np.zeros(0, np.uint32), np.zeros(1, np.int32), np.zeros(0, np.int32))
    r = db.search_by_bow_frame(m, s.slots[1:], s.frame["kps"][:0], s.frame["desc"][:0], None, empty)
    assert r["matched_kf_feature"].shape == (4, 0) and not r["n_matches"].any() and not r["pair_status"].any()
    r = db.search_by_bow_frame(m, s.slots[1:], s.frame["kps"], s.frame["desc"], None, empty)
    assert (r["matched_kf_feature"] == -1).all() and (r["matched_point"] == -1).all() and not r["n_matches"].any() and not r["pair_status"].any()
    m.close()
    db.close()


def _untouched(got, i):
    return (got["matched"][i] == -1).all() and (got["matched_point"][i] == -1).all() and got["n_matches"][i] == 0


@MODES
def test_every_pair_status_and_the_first_keyframe_unusable(oracle_lib, mode):
    s = B.Scene(seed=31, n=120, n_cand=4)
    db, m = _db(s), _matcher()
    sl, k = s.slots, s.kfs
    db.set_keyframe_features([sl[1]], [k[1]["kps"][:0]])                      # candidate 0: no feature span
    db.set_keyframe_descriptors([sl[2]], [np.zeros((0, 32), np.uint8)])       # candidate 1: no descriptor block
    db.set_keyframe_bow([sl[3]], [np.zeros((0, 2), np.int64)])                # candidate 2: an empty BoW span
    got = _call(db, m, s, mode, sl[1:])
    assert got["pair_status"].tolist() == [B.PAIR_STATUS[x] for x in ("no_features", "no_block", "no_bow", "ok")]
    assert all(_untouched(got, i) for i in range(3))
    arrays = B.gather(db)
    want = _want(oracle_lib, arrays, s, mode, [sl[4]])                        # the usable one is searched as if alone
    assert np.array_equal(got["matched"][3], want["matched"][0]) and np.array_equal(got["matched_point"][3], want["matched_point"][0])
    assert got["n_matches"][3] == want["n_matches"][0] >= 10
    # the length mismatches and the BoW index
    db.set_keyframe_features([sl[1]], [k[1]["kps"]])
    db.set_keyframe_descriptors([sl[2]], [k[2]["desc"][:-2]])                 # a block two short
    db.set_keyframe_rows([sl[1]], [k[1]["row"][:-1]])                         # a row one short
    bad = k[3]["bow"].copy()
    bad[-1, 1] = len(k[3]["row"])                                             # one past the last feature
    db.set_keyframe_bow([sl[3]], [bad])
    got = _call(db, m, s, mode, sl[1:])
    assert got["pair_status"].tolist() == [B.PAIR_STATUS[x] for x in ("length_mismatch", "length_mismatch", "bow_index", "ok")]
    assert all(_untouched(got, i) for i in range(3)) and got["n_matches"][3] == want["n_matches"][0]
    m.close()
    db.close()


def test_every_status_of_the_first_keyframe_reaches_every_pair(oracle_lib):
    """The keyframe form with the first keyframe unusable in each of the five ways: every pair carries its status, every output is -1,
    every count 0, nothing reaches the device, and the call answers as before once the relation is put back."""
    import ydorbslam_amd as y
    s = B.Scene(seed=31, n=120, n_cand=4)
    sl, k0 = s.slots, s.kfs[0]
    n = len(k0["kps"])
    past = k0["bow"].copy()
    past[-1, 1] = n                                                           # one past the last feature
    none = np.zeros((0, 2), np.int64)
    stages = (("no_features", 0, lambda d: d.set_keyframe_features([sl[0]], [k0["kps"][:0]]), lambda d: d.set_keyframe_features([sl[0]], [k0["kps"]])),
              ("no_block", n, lambda d: d.set_keyframe_descriptors([sl[0]], [k0["desc"][:0]]), lambda d: d.set_keyframe_descriptors([sl[0]], [k0["desc"]])),
              ("no_bow", n, lambda d: d.set_keyframe_bow([sl[0]], [none]), lambda d: d.set_keyframe_bow([sl[0]], [k0["bow"]])),
              ("length_mismatch", n, lambda d: d.set_keyframe_rows([sl[0]], [k0["row"][:-1]]), lambda d: d.set_keyframe_rows([sl[0]], [k0["row"]])),
              ("length_mismatch", n, lambda d: d.set_keyframe_descriptors([sl[0]], [k0["desc"][:-2]]), lambda d: d.set_keyframe_descriptors([sl[0]], [k0["desc"]])),
              ("bow_index", n, lambda d: d.set_keyframe_bow([sl[0]], [past]), lambda d: d.set_keyframe_bow([sl[0]], [k0["bow"]])))
    db, m = _db(s), _matcher()
    base = _check(db, m, s, oracle_lib, 4, every=False)
    assert (base["n_matches"] >= 10).all()
    for status, n_first, stage, restore in stages:
        stage(db)
        before = m.bow_search_stats()
        got = db.search_by_bow_keyframes(m, sl[0], sl[1:], n_first, 0.6, False)
        assert (got["pair_status"] == B.PAIR_STATUS[status]).all() and len(got["pair_status"]) == 4, status
        assert got["matched_second"].shape == got["matched_point"].shape == (4, n_first), status
        assert (got["matched_second"] == -1).all() and (got["matched_point"] == -1).all() and not got["n_matches"].any(), status
        assert m.bow_search_stats() == before, status                         # no pair to search: nothing was launched
        if n_first == 0:                                                      # n_first follows the resident count: the old count is refused
            with pytest.raises(y.YdorbError, match="the first keyframe has 0 resident features, n_first is %d" % n):
                db.search_by_bow_keyframes(m, sl[0], sl[1:], n, 0.6, False)
        restore(db)
        again = _call(db, m, s, 4, sl[1:])
        assert all(np.array_equal(again[key], base[key]) for key in base), status
    m.close()
    db.close()
# ------------------------------------------------------------------------------------------------------------ the table underneath
@MODES
def test_a_bad_flag_a_row_entry_and_a_bow_span_staged_and_pending_at_the_call(oracle_lib, mode):
    s = B.Scene(seed=32, n=150, n_cand=3)
    db, m = _db(s), _matcher()
    base = _check(db, m, s, oracle_lib, mode, every=False)
    i, o = (int(v) for v in np.argwhere(base["matched"] >= 0)[0])             # a match of pair i at output element o
    p = int(base["matched_point"][i, o])
    # the matched point goes bad: nothing is exported in between, the call itself applies the delta
    db.set_points([p], [[]], [[]], [1], [0], [0], np.zeros((1, 3), f32))
    got = _call(db, m, s, mode, s.slots[1:])
    assert got["matched_point"][i, o] != p and not (got["matched_point"] == p).any()
    _check(db, m, s, oracle_lib, mode, every=False)                           # ... and the export agrees
    db.set_points([p], [[]], [[]], [0], [0], [0], np.zeros((1, 3), f32))
    assert np.array_equal(_call(db, m, s, mode, s.slots[1:])["matched"], base["matched"])
    # the row entry behind the match is cleared
    kf, feat = (s.slots[1 + i], int(base["matched"][i, o]))                   # the keyframe whose row holds p, and where
    assert B.gather(db)["kf"][kf]["row"][feat] == p
    db.set_row_entries([kf], [feat], [-1])
    got = _call(db, m, s, mode, s.slots[1:])
    assert got["matched"][i, o] != feat
    _check(db, m, s, oracle_lib, mode, every=False)
    db.set_row_entries([kf], [feat], [p])
    # a BoW span replaced: the candidate's features of one node move to a node nothing else has
    bow = s.kfs[1 + i]["bow"].copy()
    node = bow[bow[:, 1] == feat, 0][0]
    bow[bow[:, 0] == node, 0] = 999999
    bow = bow[np.argsort(bow[:, 0], kind="stable")]
    db.set_keyframe_bow([kf], [bow])
    got = _call(db, m, s, mode, s.slots[1:])
    assert got["matched"][i, o] != feat and got["n_matches"][i] < base["n_matches"][i]
    _check(db, m, s, oracle_lib, mode, every=False)
    m.close()
    db.close()


@MODES
def test_a_row_pool_and_a_bow_pool_repack_between_two_calls_and_the_same_call_twice(oracle_lib, mode):
    s = B.Scene(seed=33, n=150, n_cand=3)
    db, m = _db(s), _matcher()
    first = _check(db, m, s, oracle_lib, mode, every=False)
    again = _call(db, m, s, mode, s.slots[1:])
    assert all(np.array_equal(first[k], again[k]) for k in first)             # the same call twice
    before_b, before_r = db.bow_stats(), db.row_stats()
    spare = [k for k in range(12) if k not in s.slots][:3]
    db.set_centres(np.arange(12), np.zeros((12, 3), f32))
    for round_ in range(4):                                                   # other keyframes come and go until both pools have repacked
        db.set_keyframe_bow(spare, [s.kfs[1 + (round_ + j) % 3]["bow"] for j in range(3)])
        db.set_keyframe_rows(spare, [s.kfs[1 + (round_ + j) % 3]["row"] for j in range(3)])
        db.export_bow()
    after_b, after_r = db.bow_stats(), db.row_stats()
    assert after_b["repacks_kept"] + after_b["repacks_grown"] > before_b["repacks_kept"] + before_b["repacks_grown"]
    assert after_r["repacks_kept"] + after_r["repacks_grown"] > before_r["repacks_kept"] + before_r["repacks_grown"]
    moved = _check(db, m, s, oracle_lib, mode, every=False)
    assert all(np.array_equal(first[k], moved[k]) for k in first)
    m.close()
    db.close()


@MODES
def test_every_other_stats_struct_is_equal_across_a_call(oracle_lib, mode):
    s = B.default_scene()
    db, m = _db(s), _matcher()
    _call(db, m, s, mode, s.slots[1:])                                        # applies what loading staged: the last_* counters say so
    _call(db, m, s, mode, s.slots[1:])                                        # nothing staged any more: they read 0, as after any query
    before = _all_stats(db)
    _call(db, m, s, mode, s.slots[1:])
    assert _all_stats(db) == before
    m.close()
    db.close()


def test_create_new_points_answers_as_before_after_a_bow_search(oracle_lib):
    """The two share the record pool and its per-pair size on the matcher: a BoW search that grew it sits between two calls."""
    import mapdb_tri_support as T
    import ydorbslam_amd as y
    tri, s = T.default_scene(), B.scene("one_node")
    db, bow_db, m = y.MapDb(0, 256, 16, 1024), _db(s), _matcher()
    tri.load(db)
    first, nbs, _keep = tri.call()
    want = tri.reference(oracle_lib)
    T.assert_same(db.create_new_points(m, first, nbs), want)
    _check(bow_db, m, s, oracle_lib, 4, every=False)                          # grows the pool on the same matcher
    assert m.bow_search_stats()["pool_per_pair"] > B.POOL_PER_PAIR
    T.assert_same(db.create_new_points(m, first, nbs), want)
    arrays = B.gather(db)                                                     # and a BoW search on the triangulation scene's own handle
    got = db.search_by_bow_keyframes(m, tri.slots[0], tri.slots[1:], tri.n, 0.9, False)
    ref = B.reference(oracle_lib, arrays, 4, tri.slots[1:], 0.9, False, first=tri.slots[0])
    got["matched"] = got["matched_second"]
    B.assert_same(got, ref, 4)
    T.assert_same(db.create_new_points(m, first, nbs), want)
    m.close()
    db.close()
    bow_db.close()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refused_up_front_with_every_stats_struct_and_the_next_result_unchanged(oracle_lib):
    import ydorbslam_amd as y
    s = B.default_scene()
    db, m = _db(s), _matcher()
    base4, base3 = _call(db, m, s, 4, s.slots[1:]), _call(db, m, s, 3, s.slots[1:])
    db.set_row_entries([s.slots[0]], [0], [s.kfs[0]["row"][0]])               # a staged delta that a refused call must leave staged
    stats, mstats = _all_stats(db), m.bow_search_stats()
    n_kf, n1, cands = db.n_keyframes, len(s.kfs[0]["kps"]), s.slots[1:]
    kps, desc, valid, fv = s.frame_args()
    refusals = [
        (lambda: db.search_by_bow_keyframes(m, n_kf, cands, n1), "first_kf_slot: keyframe slot %d outside 0..%d" % (n_kf, n_kf - 1)),
        (lambda: db.search_by_bow_keyframes(m, s.slots[0], [cands[0], -1], n1), r"second_kf_slots\[1\]: keyframe slot -1 outside"),
        (lambda: db.search_by_bow_keyframes(m, s.slots[0], cands, n1 - 1), "the first keyframe has %d resident features, n_first is %d" % (n1, n1 - 1)),
        (lambda: db.search_by_bow_keyframes(m, s.slots[0], cands, n1, ratio=float("nan")), "ratio is not finite"),
        (lambda: db.search_by_bow_keyframes(m, s.slots[0], cands, n1, ratio=float("inf")), "ratio is not finite"),
        (lambda: db.search_by_bow_frame(m, [cands[0], n_kf], kps, desc, valid, fv), r"kf_slots\[1\]: keyframe slot %d outside" % n_kf),
        (lambda: db.search_by_bow_frame(m, cands, kps, desc, valid, fv, ratio=float("-inf")), "ratio is not finite"),
        (lambda: db.search_by_bow_frame(m, cands, kps, desc, valid, y.FeatureVector(fv.node_ids, fv.node_start + 1, fv.feat)), r"frame: node_start\[0\] is 1, not 0"),
        (lambda: db.search_by_bow_frame(m, cands, kps, desc, valid, y.FeatureVector(fv.node_ids[::-1], fv.node_start, fv.feat)), "the node ids ascend strictly"),
        (lambda: db.search_by_bow_frame(m, cands, kps, desc, valid, y.FeatureVector(fv.node_ids, fv.node_start[::-1], fv.feat)), "frame: node_start"),
        (lambda: db.search_by_bow_frame(m, cands, kps, desc, valid, y.FeatureVector(fv.node_ids, fv.node_start, np.where(np.arange(len(fv.feat)) == 5, len(kps), fv.feat))),
         "frame: entry 5: feature index %d outside 0..%d" % (len(kps), len(kps) - 1)),
    ]
    for call, text in refusals:
        with pytest.raises(y.YdorbError, match=text):
            call()
    L = y.lib()
    out = np.zeros(4 * 400, np.int32)
    p = out.ctypes.data_as(C.c_void_p)
    sl = np.ascontiguousarray(cands, np.int32)
    ps = sl.ctypes.data_as(C.c_void_p)
    frame = y._lib.YdBowSide(kps.ctypes.data_as(C.c_void_p), desc.ctypes.data_as(C.c_void_p), None, len(kps), fv.c())
    big = y._lib.YdBowSide(kps.ctypes.data_as(C.c_void_p), desc.ctypes.data_as(C.c_void_p), None, 65536, fv.c())
    for fn, args, text in ((L.ydorb_mapdb_search_by_bow_keyframes, (None, m._h, 0, ps, 4, 0.6, 0, n1, p, p, p, p), "null handle"),
                           (L.ydorb_mapdb_search_by_bow_keyframes, (db._h, None, 0, ps, 4, 0.6, 0, n1, p, p, p, p), "null handle"),
                           (L.ydorb_mapdb_search_by_bow_keyframes, (db._h, m._h, s.slots[0], None, 4, 0.6, 0, n1, p, p, p, p), "null second_kf_slots"),
                           (L.ydorb_mapdb_search_by_bow_keyframes, (db._h, m._h, s.slots[0], ps, 4, 0.6, 0, n1, None, p, p, p), "null second_kf_slots, matched_second"),
                           (L.ydorb_mapdb_search_by_bow_keyframes, (db._h, m._h, s.slots[0], ps, 4, 0.6, 0, n1, p, p, p, None), "null second_kf_slots, matched_second"),
                           (L.ydorb_mapdb_search_by_bow_keyframes, (db._h, m._h, s.slots[0], ps, -1, 0.6, 0, n1, p, p, p, p), "negative number of second keyframes"),
                           (L.ydorb_mapdb_search_by_bow_keyframes, (db._h, m._h, s.slots[0], ps, 4, 0.6, 0, -1, p, p, p, p), "negative n_first"),
                           (L.ydorb_mapdb_search_by_bow_frame, (None, m._h, ps, 4, C.byref(frame), 0.6, 0, p, p, p, p), "null handle"),
                           (L.ydorb_mapdb_search_by_bow_frame, (db._h, m._h, ps, 4, None, 0.6, 0, p, p, p, p), "null frame"),
                           (L.ydorb_mapdb_search_by_bow_frame, (db._h, m._h, None, 4, C.byref(frame), 0.6, 0, p, p, p, p), "null kf_slots"),
                           (L.ydorb_mapdb_search_by_bow_frame, (db._h, m._h, ps, 4, C.byref(frame), 0.6, 0, p, None, p, p), "null kf_slots, matched_kf_feature"),
                           (L.ydorb_mapdb_search_by_bow_frame, (db._h, m._h, ps, -2, C.byref(frame), 0.6, 0, p, p, p, p), "negative number of keyframes"),
                           (L.ydorb_mapdb_search_by_bow_frame, (db._h, m._h, ps, 4, C.byref(big), 0.6, 0, p, p, p, p), "frame: n 65536 outside 0..65535")):
        assert fn(*args) == -1 and text.encode() in L.ydorb_last_error(), text
    assert _all_stats(db) == stats and m.bow_search_stats() == mstats         # nothing applied, nothing counted
    for mode, base in ((4, base4), (3, base3)):
        got = _call(db, m, s, mode, s.slots[1:])
        assert all(np.array_equal(got[k], base[k]) for k in base)
    m.close()
    db.close()


def test_a_handle_without_features_or_bow_and_too_many_pairs_refuse_and_change_nothing(oracle_lib):
    """Refused before any device work: the refusing handle's stats structs, the matcher's counters and the next result on a handle that
    has everything stay as they were."""
    import ydorbslam_amd as y
    s = B.default_scene()
    full, m = _db(s), _matcher()
    base4, base3 = _call(full, m, s, 4, s.slots[1:]), _call(full, m, s, 3, s.slots[1:])
    mstats = m.bow_search_stats()
    for enable, text in ((lambda d: d.enable_bow(), "keyframe features are not enabled"), (lambda d: d.enable_features(), "keyframe BoW feature vectors are not enabled")):
        db = _db()
        enable(db)
        db.set_centres(np.arange(8), np.zeros((8, 3), f32))
        stats = _all_stats(db)
        with pytest.raises(y.YdorbError, match=text):
            db.search_by_bow_keyframes(m, s.slots[0], s.slots[1:], 300)
        with pytest.raises(y.YdorbError, match=text):
            db.search_by_bow_frame(m, s.slots[1:], *s.frame_args())
        assert _all_stats(db) == stats and m.bow_search_stats() == mstats
        db.close()
    # more pairs than the launch grid's second dimension holds: YDORB_ERR_UNSUPPORTED, whatever the slots are
    many = np.full(65536, s.slots[1], np.int32)
    full.set_row_entries([s.slots[0]], [0], [s.kfs[0]["row"][0]])             # a staged delta that the refused calls must leave staged
    stats = _all_stats(full)
    with pytest.raises(y.YdorbError, match="65536 second keyframes, more than 65535"):
        full.search_by_bow_keyframes(m, s.slots[0], many, 300)
    with pytest.raises(y.YdorbError, match="65536 keyframes, more than 65535"):
        full.search_by_bow_frame(m, many, s.frame["kps"][:0], s.frame["desc"][:0], None, y.FeatureVector(np.zeros(0, np.uint32), np.zeros(1, np.int32), np.zeros(0, np.int32)))
    L = y.lib()
    out = np.zeros(65536, np.int32)
    p = out.ctypes.data_as(C.c_void_p)
    assert L.ydorb_mapdb_search_by_bow_keyframes(full._h, m._h, s.slots[0], many.ctypes.data_as(C.c_void_p), 65536, 0.6, 0, 0, None, None, p, p) == -5   # YDORB_ERR_UNSUPPORTED
    assert _all_stats(full) == stats and m.bow_search_stats() == mstats
    for mode, base in ((4, base4), (3, base3)):
        got = _call(full, m, s, mode, s.slots[1:])
        assert all(np.array_equal(got[k], base[k]) for k in base)
    with pytest.raises(y.YdorbError, match="the first keyframe has 300 resident features, n_first is 0"):   # 65 535 pairs pass that check
        full.search_by_bow_keyframes(m, s.slots[0], many[:65535], 0)
    m.close()
    full.close()
