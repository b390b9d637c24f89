"""ydorb_mapdb_local_ba_graph on the GPU: every output compared exactly with the CPU restatement of the sequential
loops (tests/localba_ref/localba_ref.cpp): counts, pose_kf, point_slot, every edge array, the bit patterns of points, pose_fixed and the
statuses.  tests/test_mapdb_lba_cpu.py proves on the reference alone that the scenes meet the conditions these tests rely on."""
import ctypes as C

import numpy as np
import pytest

import mapdb_lba_support as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene():
    return S.Scene()


@pytest.fixture(scope="module")
def want(scene):
    return S.ref_graph(scene.tables(), scene.kf_slots)


@pytest.fixture()
def db(scene):
    from ydorbslam_amd.map_resident import MapDb
    d = scene.load(MapDb(0, 256, 16, 1024))
    yield d
    d.close()


def check(db, kf_slots, tables):
    got = db.local_ba_graph(kf_slots, S.SIGMA)
    S.same_graph(got, S.ref_graph(tables, kf_slots))
    return got


def test_default_scene_equals_the_reference(db, scene, want):
    assert all(v == 0 for v in db.lba_stats().values())
    got = db.local_ba_graph(scene.kf_slots, S.SIGMA)
    S.same_graph(got, want)
    S.same_graph(got, S.ref_graph(S.exported(db), scene.kf_slots))     # and the device's tables are the scene's
    st = db.lba_stats()
    assert (st["n_calls"], st["last_launches"], st["last_syncs"]) == (1, 10, 2)
    assert (st["last_n_local"], st["last_n_fixed"], st["last_n_points"], st["last_n_edges"]) == (6, want["n_fixed"], len(want["point_slot"]), len(want["edge_pose"]))
    assert 0 < st["last_upload_bytes"] <= 128 and st["last_download_bytes"] < 64 * len(want["edge_pose"]) + 64 * len(want["point_slot"]) + 4096


def test_same_call_twice_then_another_list(db, scene, want):
    S.same_graph(db.local_ba_graph(scene.kf_slots, S.SIGMA), want)
    S.same_graph(db.local_ba_graph(scene.kf_slots, S.SIGMA), want)
    for kf in ([4, 1], [20, 3, 50], list(range(6, 30)), [5, 4, 3, 2, 1, 0]):
        check(db, kf, scene.tables())
    S.same_graph(db.local_ba_graph(scene.kf_slots, S.SIGMA), want)


def test_fixed_become_local_and_local_become_fixed(db, scene, want):
    """List A, then a list B in which A's fixed keyframes are local and A's local ones fixed: stale first / poseOf entries would show."""
    a, b = scene.kf_slots, want["pose_kf"][6:12]
    S.same_graph(db.local_ba_graph(a, S.SIGMA), want)
    gb = check(db, b, scene.tables())
    assert np.isin(a, gb["pose_kf"][gb["n_local"]:]).sum() >= 3
    S.same_graph(db.local_ba_graph(a, S.SIGMA), want)


def test_keyframe_without_a_row_and_rows_of_bad_points_only(db, scene):
    t = scene.tables()
    rows = list(t["rows"])
    rows[2] = np.zeros(0, np.int32)
    db.set_keyframe_rows([2], [rows[2]])
    t = dict(t, rows=rows)
    g = check(db, scene.kf_slots, t)
    assert g["n_local"] == 6 and g["pose_kf"][2] == 2
    db.set_positions([0], scene.pos[[0]])                          # something staged: the call applies it and launches nothing of its own
    g = check(db, [2], t)
    assert (g["n_local"], g["n_fixed"], len(g["point_slot"]), len(g["edge_pose"])) == (1, 0, 0, 0)
    st = db.lba_stats()
    assert (st["last_launches"], st["last_syncs"], st["last_n_local"], st["last_n_points"]) == (0, 0, 1, 0) and db.stats()["last_sync_bytes"] > 0
    bad = t["bad"].copy()
    mine = rows[4][rows[4] >= 0]
    bad[mine] = 1
    n = len(mine)
    db.set_points(mine, [scene.views[p][:, 0] for p in mine], [np.zeros(len(scene.views[p]), np.uint8) for p in mine], np.ones(n, np.uint8), np.zeros(n, np.int32),
                  np.zeros(n, np.uint8), scene.pos[mine])
    g = check(db, [4], dict(t, bad=bad))
    assert (g["n_local"], g["n_fixed"], len(g["point_slot"]), len(g["edge_pose"])) == (1, 0, 0, 0) and list(g["pose_kf"]) == [4] and list(g["pose_fixed"]) == [0]


def test_one_keyframe_and_none(db, scene):
    g = check(db, [3], scene.tables())
    assert g["n_local"] == 1 and len(g["edge_pose"]) > 50
    before = db.lba_stats()
    db.set_positions([0], scene.pos[[0]])
    g = db.local_ba_graph([], S.SIGMA)                             # an empty list leaves what is staged staged
    assert (g["n_local"], g["n_fixed"]) == (0, 0) and all(len(g[k]) == 0 for k in S.GRAPH_KEYS)
    st = db.lba_stats()
    assert st["n_calls"] == before["n_calls"] + 1 and st["last_launches"] == 0 and st["last_syncs"] == 0


def test_view_past_the_feature_length(db, scene, want):
    p = int(want["point_slot"][300])
    views = [v.copy() for v in scene.views]
    j = int(np.flatnonzero([len(scene.feats[k][0]) > 0 for k in views[p][:, 0]])[0])
    views[p][j, 1] = len(scene.feats[views[p][j, 0]][0])          # the first index past the keyframe's features
    db.set_point_views([p], [views[p]])
    g = check(db, scene.kf_slots, dict(scene.tables(), views=views))
    assert g["point_status"][300] & S.VIEW_OUT_OF_RANGE and len(g["edge_pose"]) == len(want["edge_pose"]) - 1
    keep = want["edge_point"] != 300
    assert np.array_equal(g["edge_idx"][g["edge_point"] != 300], want["edge_idx"][keep])       # nothing else changes
    assert np.array_equal(np.delete(g["point_status"], 300), np.delete(want["point_status"], 300))


def test_view_past_the_feature_length_as_a_keyframes_first_and_only_occurrence(db, scene, want):
    """The keyframe stays fixed where it was first met (rule 3 counts occurrences, whatever their idx) and only the edge goes; a keyframe
    whose only view from the local points is out of range keeps a pose and has no edge."""
    first = S.first_occurrence(want)
    views = [v.copy() for v in scene.views]
    k_first = int(want["pose_kf"][7])                               # a fixed keyframe: its first occurrence becomes out of range
    rank, _ = first[k_first]
    p = int(want["point_slot"][rank])
    j = int(np.flatnonzero(views[p][:, 0] == k_first)[0])
    views[p][j, 1] = len(scene.feats[k_first][0]) + 5
    k_only = int(scene.views[5][69, 0])                            # a sparse keyframe: the 70-view point is its only observer
    assert sum((v[:, 0] == k_only).sum() for v in scene.views) == 1 and k_only in want["pose_kf"]
    views[5][69, 1] = len(scene.feats[k_only][0])
    db.set_point_views([p, 5], [views[p], views[5]])
    g = check(db, scene.kf_slots, dict(scene.tables(), views=views))
    assert np.array_equal(g["pose_kf"], want["pose_kf"]) and np.array_equal(g["pose_fixed"], want["pose_fixed"])   # the pose list does not change
    assert len(g["edge_pose"]) == len(want["edge_pose"]) - 2 and not (g["edge_kf"] == k_only).any()
    keep = ~(((want["edge_kf"] == k_first) & (want["edge_point"] == rank)) | (want["edge_kf"] == k_only))
    for key in ("edge_pose", "edge_point", "edge_kf", "edge_idx"):
        assert np.array_equal(g[key], want[key][keep]), key
    big = int(np.flatnonzero(want["point_slot"] == 5)[0])
    changed = np.zeros(len(want["point_status"]), bool)
    changed[[rank, big]] = True
    assert (g["point_status"][changed] & S.VIEW_OUT_OF_RANGE).all() and np.array_equal(g["point_status"][~changed], want["point_status"][~changed])


def test_features_erased_between_two_calls(db, scene, want):
    S.same_graph(db.local_ba_graph(scene.kf_slots, S.SIGMA), want)
    k = int(want["pose_kf"][8])                                   # a fixed keyframe
    from ydorbslam_amd.extractor import KP_DTYPE
    feats = list(scene.feats)
    feats[k] = (np.zeros(0, KP_DTYPE), np.zeros(0, np.float32))
    db.set_keyframe_features([k], [feats[k][0]], [feats[k][1]])
    g = check(db, scene.kf_slots, dict(scene.tables(), feats=feats))
    assert k not in g["pose_kf"] and g["n_fixed"] == want["n_fixed"] - 1
    assert len(g["edge_pose"]) == len(want["edge_pose"]) - int((want["edge_kf"] == k).sum())


def test_deltas_staged_at_the_call(db, scene, want):
    """A new row, a single row entry, new views, new features and a moved position, all staged and applied by the query itself."""
    S.same_graph(db.local_ba_graph(scene.kf_slots, S.SIGMA), want)
    t = scene.tables()
    rows, views, feats, pos = list(t["rows"]), [v.copy() for v in t["views"]], list(t["feats"]), t["pos"].copy()
    far = np.arange(700, 760, dtype=np.int32)                      # points no local row held so far
    rows[1] = np.concatenate([rows[1][:150], far[:30], np.full(10, -1, np.int32)]).astype(np.int32)
    db.set_keyframe_rows([1], [rows[1]])
    free = int(np.flatnonzero(rows[3] < 0)[0])
    rows[3] = rows[3].copy()
    rows[3][free] = 745
    db.set_row_entries([3], [free], [745])
    views[745] = np.concatenate([views[745], [[3, free]]]).astype(np.int32)
    views[710] = views[710][::-1].copy()
    db.set_point_views([745, 710], [views[745], views[710]])
    r = np.random.default_rng(9)
    kp, rx = feats[20][0].copy(), feats[20][1].copy()
    kp["x"] = r.uniform(0, 640, len(kp)).astype(np.float32)
    kp["octave"] = r.integers(0, 8, len(kp))
    feats[20] = (kp, rx)
    db.set_keyframe_features([20], [kp], [rx])
    moved = want["point_slot"][[0, 257, 600]]
    pos[moved] += np.float32(0.125)
    db.set_positions(moved, pos[moved])
    model = dict(rows=rows, views=views, feats=feats, bad=t["bad"], pos=pos)
    g = check(db, scene.kf_slots, model)
    assert 745 in g["point_slot"] and len(g["point_slot"]) > len(want["point_slot"])
    S.same_graph(g, S.ref_graph(S.exported(db), scene.kf_slots))


def test_view_pool_and_feature_pool_repacks_between_two_calls(db, scene, want):
    S.same_graph(db.local_ba_graph(scene.kf_slots, S.SIGMA), want)
    d0, f0 = db.desc_stats(), db.feat_stats()
    n = scene.n_points
    for _ in range(3):                                            # every span staged again: the old ones become garbage until a repack
        db.set_point_views(np.arange(n), scene.views)
        db.set_keyframe_features(np.arange(scene.n_kf), [f[0] for f in scene.feats], [f[1] for f in scene.feats])
        S.same_graph(db.local_ba_graph(scene.kf_slots, S.SIGMA), want)
    d1, f1 = db.desc_stats(), db.feat_stats()
    assert d1["view_repacks_kept"] + d1["view_repacks_grown"] > d0["view_repacks_kept"] + d0["view_repacks_grown"]
    assert f1["repacks_kept"] + f1["repacks_grown"] > f0["repacks_kept"] + f0["repacks_grown"]


def test_all_monocular_handle():
    from ydorbslam_amd.map_resident import MapDb
    s = S.Scene(seed=2, mono_all=True)
    d = s.load(MapDb(0, 256, 16, 1024))
    try:
        g = check(d, s.kf_slots, s.tables())
        assert len(g["edge_pose"]) > 1000 and (g["edge_meas"][:, 2] == -1.0).all()
    finally:
        d.close()


def test_every_refusal_leaves_the_handle_and_the_result_as_they_were(db, scene, want):
    from ydorbslam_amd._lib import YdLocalBaGraph, lib
    from ydorbslam_amd.map_resident import MapDb
    L = lib()
    g = YdLocalBaGraph()
    kf = np.ascontiguousarray(scene.kf_slots)
    sig = S.SIGMA
    assert L.ydorb_mapdb_local_ba_graph(db._h, S._p(kf), len(kf), S._p(sig), C.byref(g)) == 0
    first_edges = np.ctypeslib.as_array(C.cast(g.problem.edge_pose, C.POINTER(C.c_int32)), (g.problem.n_edges,)).copy()
    stats = db.lba_stats()
    other = [db.stats(), db.row_stats(), db.desc_stats(), db.feat_stats()]
    bad = YdLocalBaGraph()
    twice, outside, negative = np.array([3, 1, 4, 1], np.int32), np.array([1, scene.n_kf], np.int32), np.array([-1, 1], np.int32)
    for args, text in (((S._p(kf), len(kf), S._p(sig), None), b"null out"), ((S._p(kf), -1, S._p(sig), C.byref(bad)), b"negative number of keyframe slots: -1"),
                       ((None, 2, S._p(sig), C.byref(bad)), b"null kf_slots"), ((S._p(kf), len(kf), None, C.byref(bad)), b"null inv_level_sigma2"),
                       ((S._p(outside), 2, S._p(sig), C.byref(bad)), b"kf_slots[1]: keyframe slot %d outside 0..%d" % (scene.n_kf, scene.n_kf - 1)),
                       ((S._p(negative), 2, S._p(sig), C.byref(bad)), b"kf_slots[0]: keyframe slot -1 outside"),
                       ((S._p(twice), 4, S._p(sig), C.byref(bad)), b"kf_slots[3]: keyframe slot 1 is named twice")):
        assert L.ydorb_mapdb_local_ba_graph(db._h, *args) == -1 and text in L.ydorb_last_error(), text
        assert db.lba_stats() == stats and [db.stats(), db.row_stats(), db.desc_stats(), db.feat_stats()] == other
        assert np.array_equal(np.ctypeslib.as_array(C.cast(g.problem.edge_pose, C.POINTER(C.c_int32)), (g.problem.n_edges,)), first_edges)
    assert bad.problem.n_edges == 0 and not bad.pose_kf
    S.same_graph(db.local_ba_graph(scene.kf_slots, S.SIGMA), want)
    plain = scene.load(MapDb(0, 256, 16, 1024), features=False)    # a handle that never enabled the features
    try:
        assert L.ydorb_mapdb_local_ba_graph(plain._h, S._p(kf), len(kf), S._p(sig), C.byref(bad)) == -1
        assert b"keyframe features are not enabled" in L.ydorb_last_error()
        assert all(v == 0 for v in plain.lba_stats().values()) and plain.feat_stats()["enabled"] == 0
    finally:
        plain.close()


def test_the_query_leaves_every_other_stats_struct_alone(db, scene, want):
    S.exported(db)                                                # applies what is staged
    snap = lambda: [db.stats(), db.row_stats(), db.desc_stats(), db.feat_stats(), db.bow_stats(), db.attr_stats()]
    before = snap()
    S.same_graph(db.local_ba_graph(scene.kf_slots, S.SIGMA), want)
    assert snap() == before
    got = db.points_of_keyframes(scene.kf_slots)                  # the rows query shares first / seenStamp with it
    assert np.array_equal(got["slots"], want["point_slot"])


def test_the_rows_seeded_sequence_keeps_every_earlier_stats_struct_at_a_plain_handles_values(tmp_path):
    """The rows' seeded sequence (tests/cpu_harness/mapdb_rows_check.cpp) through two handles: one answers a local_ba_graph call after every
    round, the plain one never makes one.  The row counters equal the check program's trace on both, every stats struct the handle had
    before this query is equal between the two after every round, and points_of_keyframes, which shares its kernels and its first /
    seenStamp tables with the query, gives the same answer on both."""
    import mapdb_rows_support as R
    from ydorbslam_amd.map_resident import MapDb
    rounds = R.sequence(str(tmp_path))
    traces = [r[-1][1] for r in rounds]
    handles = [MapDb(0, *R.SEQUENCE_CAPACITIES) for _ in range(2)]
    db, plain = handles
    n, n_kf = R.SEQUENCE_POINTS, 4
    obs = [np.array(sorted({p % n_kf, (7 * p + 1) % n_kf}), np.int32) for p in range(n)]
    flag = (np.arange(n) % 9 == 0).astype(np.uint8)
    for h in handles:
        h.enable_features()
        h.set_centres(np.arange(n_kf), np.zeros((n_kf, 3), np.float32))
        h.set_points(np.arange(n), obs, [np.zeros(len(o), np.uint8) for o in obs], flag, [o[0] for o in obs], np.zeros(n, np.uint8), np.zeros((n, 3), np.float32))
    snap = lambda h: [h.stats(), h.row_stats(), h.desc_stats(), h.attr_stats(), h.feat_stats(), h.bow_stats()]
    model, calls = R.RowModel(), 0
    for i, ops in enumerate(rounds):
        for op in ops[:-1]:
            model.apply(op)
            for h in handles:
                model.send(h, op)
        for h in handles:
            rows = h.export_rows()                                 # the round's one sync
            got = h.row_stats()
            assert {k: got[k] for k in R.TRACE_FIELDS[2:]} == {k: traces[i][k] for k in R.TRACE_FIELDS[2:]}, i
        kf = np.arange(len(rows), dtype=np.int32)[::-1][:12]
        g = db.local_ba_graph(kf, S.SIGMA)
        calls += 1
        plain.export()                                         # a sync with nothing staged, as the query's was
        assert snap(db) == snap(plain), i
        a, b = db.points_of_keyframes(kf), plain.points_of_keyframes(kf)
        assert np.array_equal(a["slots"], b["slots"]) and np.array_equal(g["point_slot"], a["slots"]), i
        assert snap(db) == snap(plain), i
    assert db.lba_stats()["n_calls"] == calls and all(v == 0 for v in plain.lba_stats().values())
    for h in handles:
        h.close()


def test_profiling_switch_fills_the_phase_times_and_changes_nothing_else(db, scene, want):
    S.same_graph(db.local_ba_graph(scene.kf_slots, S.SIGMA), want)
    off = db.lba_stats()
    assert all(off[k] == 0 for k in off if k.startswith("last_ms_"))
    db.lba_set_profiling(True)
    S.same_graph(db.local_ba_graph(scene.kf_slots, S.SIGMA), want)
    on = db.lba_stats()
    assert all(0 < on[k] < 100 for k in on if k.startswith("last_ms_")), on
    assert {k: v for k, v in on.items() if not k.startswith("last_ms_") and k != "n_calls"} == {k: v for k, v in off.items() if not k.startswith("last_ms_") and k != "n_calls"}
    db.lba_set_profiling(False)
    S.same_graph(db.local_ba_graph(scene.kf_slots, S.SIGMA), want)
    assert all(db.lba_stats()[k] == 0 for k in on if k.startswith("last_ms_"))


# ------------------------------------------------------------------------------------------------------------ hand-over to the solver
def _solve(prob):
    from ydorbslam_amd.optimizer import Optimizer
    r = Optimizer.local_bundle_adjust(prob)
    return r["poses"], r["points"], r["outlier"], r["log"]


def test_hand_over_to_the_solver_is_byte_identical():
    from ydorbslam_amd._lib import YdBaResult, YdLocalBaGraph, lib
    from ydorbslam_amd.map_resident import MapDb
    s, poses, camera = S.solver_scene()
    d = s.load(MapDb(0, 256, 16, 1024))
    try:
        g = d.local_ba_graph(s.kf_slots, S.SIGMA)
        flat, reference = S.dict_graph(S.exported(d), s.kf_slots), S.ref_graph(s.tables(), s.kf_slots)
        S.same_graph(g, flat)
        S.same_graph(g, reference)
        results = []
        for graph in (g, flat, reference):
            graph = dict(graph, pose_fixed=np.where(graph["pose_kf"] == 0, 1, graph["pose_fixed"]).astype(np.uint8))   # keyframe id 0 is fixed
            results.append(_solve(S.problem_of(graph, poses[graph["pose_kf"]], camera)))
        # ... and the solve straight on the handle's pinned result, poses and intrinsics filled in place
        L = lib()
        G = YdLocalBaGraph()
        kf = np.ascontiguousarray(s.kf_slots)
        assert L.ydorb_mapdb_local_ba_graph(d._h, S._p(kf), len(kf), S._p(S.SIGMA), C.byref(G)) == 0
        P = G.problem
        pose_kf = np.ctypeslib.as_array(C.cast(G.pose_kf, C.POINTER(C.c_int32)), (P.n_poses,))
        np.ctypeslib.as_array(C.cast(P.poses, C.POINTER(C.c_double)), (P.n_poses, 7))[:] = poses[pose_kf]
        np.ctypeslib.as_array(C.cast(P.pose_fixed, C.POINTER(C.c_uint8)), (P.n_poses,))[pose_kf == 0] = 1
        P.fx, P.fy, P.cx, P.cy, P.bf = (float(v) for v in camera)
        out = np.zeros(P.n_edges, np.uint8)
        res = YdBaResult()
        res.edge_outlier = out.ctypes.data_as(C.c_void_p).value
        assert L.ydorb_ba_solve(C.byref(P), None, C.byref(res)) == 0, L.ydorb_last_error()
        n = res.n_log
        log = np.stack([np.array(res.log_chi2[:n]), np.array(res.log_lambda[:n]), np.array(res.log_trials[:n], np.float64), np.array(res.log_stage[:n], np.float64)], axis=1)
        results.append((np.ctypeslib.as_array(C.cast(P.poses, C.POINTER(C.c_double)), (P.n_poses, 7)).copy(),
                        np.ctypeslib.as_array(C.cast(P.points, C.POINTER(C.c_double)), (P.n_points, 3)).copy(), out, log))
        base = results[0]
        assert len(base[3]) >= 2 and base[3][-1, 0] < base[3][0, 0] and not np.array_equal(S.bits(base[0]), S.bits(poses[g["pose_kf"]]))   # the solve did something
        for other in results[1:]:
            for a, b in zip(base, other):
                assert a.shape == b.shape and np.array_equal(S.bits(a), S.bits(b))
    finally:
        d.close()
