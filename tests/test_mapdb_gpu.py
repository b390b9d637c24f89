"""The resident map table on the GPU (ydorbslam_amd/csrc/map_resident.hip): loaded by deltas, queried with no table upload, against the
flat entries and the CPU restatement (tests/mapmaint_ref) on the same table, exactly: integers, status bytes and float bit patterns.
The seeded sequence of tests/cpu_harness/mapdb_host_check.cpp runs through the real handle and must show that program's counters, so
both kinds of repack and both table growths ran on the device."""
import numpy as np
import pytest

import mapdb_support as D
import mapmaint_support as S
from test_mapmaint_gpu import SPANS

pytestmark = pytest.mark.gpu
SF = S.scale_factors()


def _db(*caps):
    from ydorbslam_amd import MapDb
    return MapDb(0, *caps)


def test_load_in_three_shuffled_calls_and_query_against_flat_entries_and_restatement():
    from ydorbslam_amd import map_maintenance as M
    m = S.random_map(5, 40, 600, 0, 12, bad_share=0.05, level_spread=1)
    T = m["table"]
    db = _db(256, 8, 1000)                                       # every table grows during the load
    D.load(db, m, np.random.default_rng(1).permutation(600), calls=3)
    D.same_export(db.export(), m)
    D.three_queries_equal_the_restatement(db, m)
    S.same_normal_depth(db.update_normal_depth(np.arange(600), SF), M.update_normal_depth(T, m["pos"], m["centre"], m["ref_kf"], m["ref_level"], SF))
    q = np.arange(40, dtype=np.int32)
    S.same_covisibility(db.covisibility(q, m["kf_points"]), M.covisibility(T, q, m["kf_points"]))
    cand, lists, own = S.candidates(m)
    removed = np.zeros(40, np.uint8)
    removed[[3, 9, 21]] = 1
    for rem in (None, removed):
        S.same_redundancy(db.keyframe_redundancy(cand, lists, own, rem), M.keyframe_redundancy(T, cand, lists, own, rem))
    s = db.stats()
    assert s["point_table_growths"] >= 1 and s["keyframe_table_growths"] >= 1 and s["repacks_grown"] >= 1
    db.close()


@pytest.fixture(scope="module")
def rounds(tmp_path_factory):
    return D.sequence(str(tmp_path_factory.mktemp("mapdbseq")))


def test_the_seeded_sequence_on_the_device_equals_the_model_and_the_cpu_trace(rounds):
    """After every round export equals the model and stats equals the CPU program's trace; on three rounds, the one before the first
    capacity-keeping repack, that round and the last, the three queries equal the restatement on the model's flat table."""
    traces = [r[-1][1] for r in rounds]
    kept = next(i for i, t in enumerate(traces) if t["repacks_kept"] == 1)
    assert kept > 1 and traces[-1]["repacks_grown"] >= 1 and traces[-1]["point_table_growths"] >= 1 and traces[-1]["keyframe_table_growths"] >= 1
    db, model = _db(*D.SEQUENCE_CAPACITIES), D.Model()
    for i, ops in enumerate(rounds):
        for op in ops[:-1]:
            model.apply(op)
            model.send(db, op)
        flat = model.flat()
        D.same_export(db.export(), flat)                          # export applies what is staged: the round's one sync
        got = db.stats()
        assert {k: got[k] for k in D.TRACE_FIELDS[1:]} == {k: traces[i][k] for k in D.TRACE_FIELDS[1:]}, i
        if i in (kept - 1, kept, len(rounds) - 1):
            D.three_queries_equal_the_restatement(db, flat)
            assert db.stats()["last_sync_bytes"] == 0              # the queries found nothing staged
    db.close()


def _span_mix(n_points, n_kf=320, seed=4):
    """test_mapmaint_gpu's span mix: 0, 1, 63, 64, 65 and 300 observers among others, every seventh point bad, points 2 and 8 on a centre."""
    from test_mapmaint_gpu import normal_scene
    T, pos, centre, ref_kf, ref_level, sf = normal_scene(n_points, 8, seed)
    return dict(table=T, pos=pos, centre=centre, ref_kf=ref_kf, ref_level=ref_level), sf


def test_subset_normals_in_the_order_given_with_a_repeat_and_a_never_set_slot():
    m, sf = _span_mix(1000)
    assert SPANS[1] == 0 and {63, 64, 65, 300} <= set(SPANS)
    want = S.ref_update_normal_depth(m["table"], m["pos"], m["centre"], m["ref_kf"], m["ref_level"], sf)
    T = m["table"]
    keep = np.setdiff1d(np.arange(1000), [502])                   # slot 502 (one observer, not bad) is never set
    live = int(T.obs_start[-1]) - 1
    db = _db(1100, 320, live + 100)                               # the pool holds the load and little more
    D.load(db, m, keep)
    rng = np.random.default_rng(9)
    for n in (1, 63, 64, 65, 257):
        slots = rng.permutation(keep)[:n].astype(np.int32)
        if n == 1:
            slots[0] = 2                                          # the point on its only observer's centre: NaN, as in the reference
        if n == 65:
            slots[7], slots[40] = 502, 16                         # never set; 16 has 300 observers
        if n == 257:
            slots[100] = slots[3]                                 # a repeated slot
            slots[:10] = np.arange(10)                            # every span length of the mix
        got = db.update_normal_depth(slots, sf)
        pick = {k: v[slots].copy() for k, v in want.items()}
        if n == 65:
            pick["status"][7] = 1                                 # YDORB_MAP_BAD, zeros
            for k in ("normal", "min_distance", "max_distance"):
                pick[k][7] = 0
        S.same_normal_depth(got, pick)
        if n == 257:
            assert {0, 1, 2} == set(got["status"].tolist()) and np.isnan(got["normal"][2]).all()
    # a repack that moves this mix: the short spans are re-sent, the pool has no room, and the spans of 63 (copied by a lane) and of 64,
    # 65 and 300 (copied by a wave) survive into the new arena
    before = db.stats()
    D.load(db, m, keep[np.isin(keep % 10, [0, 1, 2, 7, 8, 9])])
    S.same_normal_depth(db.update_normal_depth(keep, sf), {k: v[keep] for k, v in want.items()})
    after = db.stats()
    assert after["repacks_grown"] == before["repacks_grown"] + 1 and after["pool_used"] == live == after["n_observations"]
    mask = np.ones(len(T.obs_kf), bool)
    mask[T.obs_start[502]:T.obs_start[503]] = False
    back = db.export()["table"]
    assert np.array_equal(back.obs_kf, T.obs_kf[mask]) and np.array_equal(back.obs_level, T.obs_level[mask])
    assert np.array_equal(np.diff(back.obs_start), np.where(np.arange(1000) == 502, 0, np.diff(T.obs_start)))
    db.close()


def test_covisibility_across_a_window_boundary_and_its_capacity():
    from ydorbslam_amd import map_maintenance as M
    from test_mapmaint_gpu import covis_scene
    W = M.COVIS_WINDOW
    T, query, lists = covis_scene(W + 1, 1)
    obs, lev = D.split_levels(T)
    db = _db(64, W + 1, 1024)
    db.set_centres(np.arange(W + 1), np.zeros((W + 1, 3), np.float32))
    db.set_points(np.arange(36), obs, lev, T.bad, np.zeros(36, np.int32), np.zeros(36, np.uint8), np.zeros((36, 3), np.float32))
    want = S.ref_covisibility(T, query, lists)
    S.same_covisibility(db.covisibility(query, lists), want)
    assert want[0]["kf"].min() < W <= want[0]["kf"].max()        # connections on both sides of the window boundary
    exact = [want[0]["count"]]
    fits = db.covisibility(query, lists, exact)
    S.same_covisibility(fits, S.ref_covisibility(T, query, lists, exact))
    assert fits[0]["status"] == 0 and len(fits[0]["kf"]) == exact[0]
    short = db.covisibility(query, lists, [exact[0] - 1])
    S.same_covisibility(short, S.ref_covisibility(T, query, lists, [exact[0] - 1]))
    assert short[0]["status"] == 1 and short[0]["count"] == exact[0] and (short[0]["raw_kf"] == -1).all()
    db.close()


def test_culling_boundaries_and_the_masked_walk_over_the_resident_entry():
    table, cand, lists, own, want = S.boundary_table()
    obs, lev = D.split_levels(table)
    n = table.n_points
    db = _db(8, 4, 16)
    db.set_centres(np.arange(12), np.zeros((12, 3), np.float32))
    db.set_points(np.arange(n), obs, lev, table.bad, np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros((n, 3), np.float32))
    r = db.keyframe_redundancy(cand, lists, own)
    assert list(r["n_counted"]) == want["n_counted"] and list(r["n_redundant"]) == want["n_redundant"] and list(r["cull"]) == want["cull"]
    db.close()
    m = S.culling_map(S.CULLING_SEEDS[0])
    db = _db(600, 40, 8192)
    D.load(db, m)
    cand, lists, own = S.candidates(m)
    seq = S.ref_sequential_culling(m["table"], cand, lists, own)
    msk = S.masked_culling(lambda _t, c, l, o, rem, th: db.keyframe_redundancy(c, l, o, rem, th), m["table"], cand, lists, own)
    assert int(seq["erased"].sum()) >= 2 and msk["calls"] >= 3
    for k in ("verdict", "erased", "n_counted", "n_redundant"):
        assert np.array_equal(seq[k], msk[k]), k
    db.close()


def test_resident_list_queries_refuse_bad_arguments_with_the_flat_entries_words():
    """Covisibility and redundancy through the C ABI, flat and resident, on one table of 3 points over 4 keyframe slots: every bad call
    is YDORB_ERR_INVALID_ARG on both routes, with the same message behind the route's prefix."""
    import ctypes as C
    from ydorbslam_amd import map_maintenance as M
    from ydorbslam_amd._lib import lib
    T = M.ObservationTable(4, [[0, 1], [1, 2, 3], [0]], [[0, 1], [1, 0, 2], [0]])
    obs, lev = D.split_levels(T)
    db = _db(4, 4, 16)
    db.set_centres(np.arange(4), np.zeros((4, 3), np.float32))
    db.set_points(np.arange(3), obs, lev, T.bad, np.zeros(3, np.int32), np.zeros(3, np.uint8), np.zeros((3, 3), np.float32))
    i32 = lambda *v: np.array(v, np.int32)
    out = lambda: np.zeros(4, np.int32)
    good_c = dict(kf=i32(0, 1), n=2, ls=i32(0, 1, 2), idx=i32(0, 1), os=i32(0, 3, 6), conn=np.zeros(6, np.int32), w=np.zeros(6, np.int32),
                  counts=out(), status=np.zeros(4, np.uint8))
    good_r = dict(kf=i32(0, 1), n=2, ls=i32(0, 1, 2), idx=i32(0, 1), own=np.zeros(2, np.uint8), nc=out(), nr=out(), cull=np.zeros(4, np.uint8))

    def covis(a, resident):
        tail = (M._p(a["conn"]), M._p(a["w"]), M._p(a["counts"]), M._p(a["status"]))
        head = (M._p(a["kf"]), a["n"], M._p(a["ls"]), M._p(a["idx"]), M._p(a["os"]))
        return lib().ydorb_mapdb_covisibility(db._h, *head, *tail) if resident else lib().ydorb_map_covisibility(C.byref(T.struct), *head, 0, *tail)

    def redundancy(a, resident):
        tail = (M._p(a["nc"]), M._p(a["nr"]), M._p(a["cull"]))
        head = (M._p(a["kf"]), a["n"], M._p(a["ls"]), M._p(a["idx"]), M._p(a["own"]), None, 3)
        return lib().ydorb_mapdb_keyframe_redundancy(db._h, *head, *tail) if resident else lib().ydorb_map_keyframe_redundancy(C.byref(T.struct), *head, 0, *tail)

    assert covis(good_c, False) == 0 and covis(good_c, True) == 0 and redundancy(good_r, False) == 0 and redundancy(good_r, True) == 0
    bad = [(covis, dict(good_c, kf=i32(4, 1)), "query_kf[0]: keyframe slot 4 outside 0..3"),
           (covis, dict(good_c, idx=i32(0, 3)), "list entry 1: point index 3 outside the table of 3"),
           (covis, dict(good_c, os=i32(0, 3, 2)), "out_start decreases at 2: 2 after 3"),
           (covis, dict(good_c, counts=None), "null counts or status"),
           (covis, dict(good_c, conn=None), "null conn_kf or conn_weight"),
           (redundancy, dict(good_r, kf=i32(0, 4)), "cand_kf[1]: keyframe slot 4 outside 0..3"),
           (redundancy, dict(good_r, idx=i32(3, 1)), "list entry 0: point index 3 outside the table of 3"),
           (redundancy, dict(good_r, own=None), "null own_level"),
           (redundancy, dict(good_r, nc=None), "null output arrays")]
    for fn, args, words in bad:
        said = []
        for resident, prefix in ((False, "map maintenance: "), (True, "resident map table: ")):
            assert fn(args, resident) == -1, (words, resident)     # YDORB_ERR_INVALID_ARG
            text = lib().ydorb_last_error().decode()
            assert text.startswith(prefix), text
            said.append(text[len(prefix):])
        assert said[0] == said[1] == words
    db.close()


def _touch_three(db, m):
    T = m["table"]
    obs, lev = D.split_levels(T)
    db.set_points([7, 50, 99], [obs[7][:2], np.concatenate([obs[50], obs[3]]), []], [lev[7][:2], np.concatenate([lev[50], lev[3]]), []], [0, 0, 1],
                  [int(obs[7][0]), int(obs[50][0]), 0], [0, 0, 0], np.ones((3, 3), np.float32))
    return len(obs[50]) + len(obs[3])


def test_upload_accounting_does_not_grow_with_the_table():
    cost = []
    for n in (100, 10000):
        m = S.random_map(17, 20, n, 2, 6)
        db = _db(n, 20, 8 * n)
        D.load(db, m)
        first = db.update_normal_depth(np.arange(n), SF)
        loaded = db.stats()
        assert loaded["last_sync_records"] == n + 20 and loaded["last_sync_bytes"] >= 32 * n
        second = db.update_normal_depth(np.arange(n), SF)
        assert db.stats()["last_sync_bytes"] == 0 and db.stats()["last_sync_records"] == 0
        S.same_normal_depth(second, first)
        if n == 100:                                               # the spans must be the same in both tables: take them from the small one
            small = m
        payload = _touch_three(db, small)
        db.covisibility([0], [np.arange(100, dtype=np.int32)])
        s = db.stats()
        assert s["last_sync_records"] == 3
        cost.append(s["last_sync_bytes"])
        assert 3 * 32 + 5 * payload <= cost[-1] <= 3 * 32 + 5 * payload + 3 * 16      # three records, the payload, section padding
        db.close()
    assert cost[0] == cost[1]


def test_clear_then_reuse():
    a, b = S.random_map(31, 12, 150, 1, 6), S.random_map(32, 9, 80, 0, 5, bad_share=0.1)
    db = _db(64, 4, 256)
    D.load(db, a)
    D.three_queries_equal_the_restatement(db, a)
    before = db.stats()
    db.clear()
    s = db.stats()
    assert (s["n_points"], s["n_keyframes"], s["n_observations"], s["pool_used"]) == (0, 0, 0, 0)
    assert s["point_capacity"] == before["point_capacity"] and s["pool_capacity"] == before["pool_capacity"]
    D.load(db, b, np.arange(80)[::-1], calls=2)
    D.same_export(db.export(), b)
    D.three_queries_equal_the_restatement(db, b)
    db.clear()                                                     # a slot of the first map that the second never set reads as never set
    db.set_centres([0], [[0, 0, 0]])
    db.set_points([120], [[0]], [[0]], [0], [0], [0], [[1, 1, 1]])
    r = db.update_normal_depth([100, 120], SF)
    assert list(r["status"]) == [1, 0]
    db.close()


def test_two_handles_are_independent_and_identical_sequences_give_identical_bytes():
    a, b = S.random_map(41, 15, 200, 1, 8), S.random_map(42, 11, 120, 1, 5)
    one, two, twin = _db(32, 4, 64), _db(32, 4, 64), _db(32, 4, 64)
    D.load(one, a, calls=2)
    D.load(two, b)
    D.load(twin, a, calls=2)
    D.three_queries_equal_the_restatement(two, b)                  # interleaved: neither handle sees the other's table
    D.three_queries_equal_the_restatement(one, a)
    D.three_queries_equal_the_restatement(two, b)
    D.three_queries_equal_the_restatement(twin, a)                 # the twin makes the calls of `one`, so it shows its counters too
    moved =(a["pos"][:40] + np.float32(0.25)).astype(np.float32)
    for db in (one, twin):
        db.set_positions(np.arange(40), moved)
    a2 = dict(a, pos=np.concatenate([moved, a["pos"][40:]]))
    for db in (one, twin):                                         # the same calls on both, so also the same counters
        D.three_queries_equal_the_restatement(db, a2)
    D.same_export(two.export(), b)
    e1, e2 = one.export(), twin.export()
    D.same_export(e1, dict(a2, table=e2["table"]))
    D.same_export(e1, e2)
    assert one.stats() == twin.stats()
    S.same_normal_depth(one.update_normal_depth(np.arange(200), SF), twin.update_normal_depth(np.arange(200), SF))
    for db in (one, two, twin):
        db.close()
