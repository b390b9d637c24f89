"""The resident table's descriptor blocks, point views and the distinctive-descriptor query on the GPU
(ydorbslam_amd/csrc/map_resident.hip, mapdb_desc_kernels.hip.h).  The reference of every query is
oracle.orb_oracle.distinctive_descriptor on rows gathered in Python from the test's own arrays (mapdb_desc_support.DescModel); the
churn test replays the seeded sequence of tests/cpu_harness/mapdb_desc_check.cpp through the real handle and holds the exports to the
model and ydorb_mapdb_desc_stats to that program's counters.  Every comparison is exact.  At most 400 keyframes x 16 descriptors and
600 points."""
import numpy as np
import pytest

import mapcorrect_support as MC
import mapdb_desc_support as R
import mapdb_support as D
import mapmaint_support as S

pytestmark = pytest.mark.gpu
I32 = np.int32
L = R.STAGE_ROWS
COUNTS = (0, 1, 2, 3, 4, 63, 64, 65, 129, L + 1, 2 * L)   # the kth = (int)(0.5 m) corners, the 64-lane round boundary, the global fallback


def _handle(n_points, n_kf, bad=(), never=(), caps=None):
    """A handle with n_kf keyframes (centres only) and point slots 0 .. n_points-1 without observations; `never` = slots not set at all."""
    from ydorbslam_amd import MapDb
    db = MapDb(0, *(caps or (max(n_points, 1), max(n_kf, 1), 16)))
    db.set_centres(np.arange(n_kf), np.zeros((n_kf, 3), np.float32))
    slots = np.array([p for p in range(n_points) if p not in set(never)], I32)
    n = len(slots)
    none = [np.zeros(0, I32)] * n
    db.set_points(slots, none, [np.zeros(0, np.uint8)] * n, np.isin(slots, list(bad)).astype(np.uint8), np.zeros(n, I32), np.zeros(n, np.uint8),
                  np.zeros((n, 3), np.float32))
    model = R.DescModel(n_points, n_kf)
    model.bad[np.array(list(bad) + list(never), np.int64)] = 1
    return db, model


def _near(rng, base, n, flips=2):
    """n rows, each one of the base rows with up to `flips` bits flipped: equal medians are common."""
    rows = base[rng.integers(0, len(base), n)].copy()
    for r in rows:
        for _ in range(int(rng.integers(0, flips + 1))):
            r[rng.integers(0, 32)] ^= np.uint8(1 << int(rng.integers(0, 8)))
    return rows


@pytest.fixture(scope="module")
def sized():
    """One handle for the collected-row counts: 40 keyframes x 16 descriptors, keyframes 36 .. 39 without a block; point i is seen
    COUNTS[i] times in keyframes with a block, and three more times, first, in the middle and last, in keyframes without one."""
    rng = np.random.default_rng(11)
    base = rng.integers(0, 256, (4, 32)).astype(np.uint8)
    db, model = _handle(len(COUNTS), 40)
    model.send(db, blocks=(np.arange(36), [_near(rng, base, 16) for _ in range(36)]))
    views = []
    for m in COUNTS:
        v = np.stack([rng.integers(0, 36, m), rng.integers(0, 16, m)], axis=1).astype(I32)
        dead = np.stack([rng.integers(36, 40, 3), rng.integers(0, 16, 3)], axis=1).astype(I32)
        views.append(np.concatenate([dead[:1], v[:m // 2], dead[1:2], v[m // 2:], dead[2:]]))
    model.send(db, views=(np.arange(len(COUNTS)), views))
    yield db, model
    db.close()


@pytest.mark.parametrize("i", range(len(COUNTS)))
def test_collected_row_counts(sized, oracle_lib, i):
    db, model = sized
    got = model.check_query(db, [i], oracle_lib)
    assert got["status"][0] == (R.NO_DESCRIPTORS if COUNTS[i] == 0 else R.UPDATED)
    if COUNTS[i]:
        assert 1 <= got["best"][0] <= COUNTS[i] + 1                # a span position: the first view is a skipped one


def test_all_counts_in_one_call_and_in_reverse(sized, oracle_lib):
    db, model = sized
    model.check_query(db, np.arange(len(COUNTS)), oracle_lib)
    model.check_query(db, np.arange(len(COUNTS))[::-1], oracle_lib)
    assert db.desc_stats()["last_desc_sync_bytes"] == 0


def test_ties(oracle_lib):
    rng = np.random.default_rng(5)
    db, model = _handle(40, 64)
    pairs = rng.integers(0, 256, (32, 2, 32)).astype(np.uint8)     # keyframes 2j and 2j + 1 both hold [A_j, B_j]
    model.send(db, blocks=(np.arange(64), [pairs[k // 2] for k in range(64)]))
    views = [np.array([[2 * j, 0], [2 * j + 1, 0], [2 * j, 1], [2 * j + 1, 1]], I32) for j in range(32)]   # rows A A B B
    views.append(np.array([[0, 0], [1, 0], [0, 0], [1, 0], [0, 0]], I32))                                    # all rows identical
    views.append(np.array([[0, 1], [0, 0], [1, 0], [0, 0]], I32))                                            # B A A A: the winner's median is shared by later rows
    model.send(db, views=(np.arange(34), views))
    # from the oracle side alone: every one of these points has a tie for the least median
    for p in range(34):
        rows = np.stack([model.blocks[k][i] for k, i in model.views[p]])
        least, share = R.median_ties(rows)
        assert share >= 2, p
        if p < 32:
            assert share == 4
    got = model.check_query(db, np.arange(34), oracle_lib)
    assert (got["status"] == R.UPDATED).all() and (got["best"][:33] == 0).all() and got["best"][33] == 1
    db.close()


def test_skipped_views_and_position_mapping(oracle_lib):
    rng = np.random.default_rng(7)
    db, model = _handle(6, 8)
    A, B = rng.integers(0, 256, (2, 32)).astype(np.uint8)
    model.send(db, blocks=([0, 1, 2], [np.stack([A, B]), np.stack([A, B]), np.stack([B, A])]))   # keyframes 3 .. 7 hold no block
    views = [np.array([[3, 0], [4, 1], [0, 1], [5, 0], [0, 0], [1, 0], [6, 9]], I32),   # rows B A A behind two skipped views: the winner is span position 4
             np.array([[3, 0], [7, 5], [4, 0]], I32),                                   # every view skipped
             np.array([[2, 0], [7, 1]], I32),                                           # a skipped view last
             np.zeros((0, 2), I32)]                                                     # no views
    model.send(db, views=(np.arange(4), views))
    got = model.check_query(db, [0, 1, 2, 3], oracle_lib)
    assert got["status"].tolist() == [R.UPDATED, R.NO_DESCRIPTORS, R.UPDATED, R.NO_DESCRIPTORS]
    assert got["best"].tolist() == [4, -1, 0, -1] and got["best_view"][0].tolist() == [0, 0] and np.array_equal(got["desc"][0], A)
    assert not got["desc"][1].any() and not got["best_view"][1].any()
    model.send(db, blocks=([0], [np.zeros((0, 32), np.uint8)]))     # keyframe 0 culled: point 0 is left with keyframe 1's row
    got = model.check_query(db, [0, 2], oracle_lib)
    assert got["best"].tolist() == [5, 0]
    db.close()


def test_a_view_past_its_block_is_a_status_and_reads_no_row(oracle_lib):
    rng = np.random.default_rng(9)
    db, model = _handle(5, 3)
    model.send(db, blocks=([0, 1], [rng.integers(0, 256, (16, 32)).astype(np.uint8), rng.integers(0, 256, (5, 32)).astype(np.uint8)]))
    ok = np.array([[0, 3], [1, 4], [0, 15]], I32)
    views = [ok, np.array([[0, 3], [1, 5], [0, 15]], I32), ok[::-1].copy(), np.array([[2, 99], [0, 16]], I32), np.array([[2, 99]], I32)]
    model.send(db, views=(np.arange(5), views))                    # point 1: idx == len in keyframe 1; point 3: idx == len behind a skipped view
    got = model.check_query(db, [0, 1, 2, 3, 4, 1, 0], oracle_lib)  # the call returns YDORB_OK: check() raised nothing
    assert got["status"].tolist() == [R.UPDATED, R.VIEW_OUT_OF_RANGE, R.UPDATED, R.VIEW_OUT_OF_RANGE, R.NO_DESCRIPTORS, R.VIEW_OUT_OF_RANGE, R.UPDATED]
    for q in (1, 3, 5):
        assert got["best"][q] == -1 and not got["desc"][q].any() and not got["best_view"][q].any()
    alone = model.check_query(db, [0, 2], oracle_lib)                # the other points are what they are without the flagged ones
    assert np.array_equal(alone["desc"], got["desc"][[0, 2]]) and np.array_equal(alone["best"], got["best"][[0, 2]])
    db.close()


def test_bad_never_set_repeated_and_empty_queries(oracle_lib):
    from ydorbslam_amd import YdorbError
    rng = np.random.default_rng(13)
    db, model = _handle(13, 2, bad=(4,), never=(10, 11))
    model.send(db, blocks=([0, 1], [rng.integers(0, 256, (8, 32)).astype(np.uint8)] * 2))
    v = np.array([[0, 1], [1, 2], [0, 7]], I32)
    model.send(db, views=([3, 4, 10, 12], [v, v, v, v[:1]]))       # views of a bad point and of a never-set slot are held and not read
    got = model.check_query(db, [3, 4, 10, 11, 12, 3, 3, 12], oracle_lib)
    assert got["status"].tolist() == [0, R.BAD, R.BAD, R.BAD, 0, 0, 0, 0] and got["best"][4] == 0
    assert np.array_equal(got["desc"][0], got["desc"][5]) and np.array_equal(got["desc"][0], got["desc"][6])
    empty = db.distinctive_descriptors([])
    assert len(empty["best"]) == 0 and len(empty["status"]) == 0
    with pytest.raises(YdorbError, match=r"slots\[1\]: point slot 13 outside 0..12"):
        db.distinctive_descriptors([0, 13])
    with pytest.raises(YdorbError, match="keyframe slot 2 outside 0..1"):
        db.set_point_views([0], [[[2, 0]]])
    with pytest.raises(YdorbError, match="set the point before its views"):
        db.set_point_views([13], [[[0, 0]]])
    with pytest.raises(YdorbError, match="the pools are not empty"):
        db.reserve_descriptors(10, 10)
    model.check_query(db, [3, 12], oracle_lib)                      # the refused calls staged nothing
    db.clear()
    assert db.desc_stats()["n_views"] == 0 and db.desc_stats()["n_descriptors"] == 0 and db.n_points == 0
    db.reserve_descriptors(64, 64)
    assert db.desc_stats()["view_pool_capacity"] == 64 and db.desc_stats()["desc_pool_capacity"] == 64
    db.close()


def test_a_keyframe_a_point_and_its_views_staged_in_one_interval(oracle_lib):
    rng = np.random.default_rng(17)
    db, model = _handle(3, 2, caps=(4, 2, 16))
    model.send(db, blocks=([0], [rng.integers(0, 256, (4, 32)).astype(np.uint8)]), views=([0], [[[0, 1], [0, 3]]]))
    model.check_query(db, [0], oracle_lib)
    # nothing between here and the query touches the device: a new keyframe (its block names the slot), new points past the point
    # table's capacity, their views
    model.send(db, blocks=([5], [rng.integers(0, 256, (6, 32)).astype(np.uint8)]))
    assert db.n_keyframes == 6
    new = np.arange(3, 9)
    db.set_points(new, [np.zeros(0, I32)] * 6, [np.zeros(0, np.uint8)] * 6, np.zeros(6, np.uint8), np.zeros(6, I32), np.zeros(6, np.uint8), np.zeros((6, 3), np.float32))
    model.grow_points(9)
    model.send(db, views=(new, [np.array([[5, p % 6], [0, p % 4], [5, (p + 1) % 6]], I32) for p in new]))
    got = model.check_query(db, np.arange(9), oracle_lib)
    assert (got["status"][3:] == R.UPDATED).all() and db.stats()["point_table_growths"] == 1
    model.check_exports(db)
    db.close()


def test_the_seeded_sequence_on_the_device_equals_the_model_and_the_cpu_trace(tmp_path, oracle_lib):
    """Churn: blocks erased and re-added, views replaced until each pool has repacked both ways."""
    rounds = R.sequence(str(tmp_path))
    traces = [r[-1][1] for r in rounds]
    n_points = max(op[1] for r in rounds for op in r if op[0] == "P")
    first = {k: next(i for i, t in enumerate(traces) if t[k] >= 1) for k in ("view_repacks_kept", "view_repacks_grown", "desc_repacks_kept", "desc_repacks_grown")}
    db, model = _handle(n_points, R.SEQUENCE_KEYFRAMES, bad=range(5, n_points, 11), caps=(n_points, R.SEQUENCE_KEYFRAMES, 16))
    db.set_keyframe_rows([0], [[1, 2]])
    db.reserve_descriptors(*R.SEQUENCE_RESERVE)
    db.export()
    db.export_rows()
    base, base_rows = db.stats(), db.row_stats()
    assert base["last_sync_bytes"] == 0 and base_rows["last_row_sync_bytes"] == 0
    for i, ops in enumerate(rounds):
        for op in ops[:-1]:
            if op[0] == "B":
                model.send(db, blocks=op[1:])
            elif op[0] == "V":
                model.send(db, views=op[1:])
        got = model.check_exports(db)                               # the first export applies what is staged: the round's one sync
        assert {k: got[k] for k in R.TRACE_FIELDS[1:]} == {k: traces[i][k] for k in R.TRACE_FIELDS[1:]}, i
        assert db.stats() == base and db.row_stats() == base_rows   # the traffic of the two relations is in YdMapDbDescStats only
        if i in set(first.values()) | {0, 9, 10, 30, len(rounds) - 1}:
            model.check_query(db, np.arange(n_points), oracle_lib)
            assert db.desc_stats()["last_desc_sync_bytes"] == 0     # the query found nothing staged
    last = db.desc_stats()
    assert min(last[k] for k in first) >= 1
    db.close()


def test_interleaved_with_the_older_entries_on_one_handle(oracle_lib):
    """update_normal_depth, covisibility, points_of_keyframes and correct give what they give on a handle that never saw a descriptor."""
    from ydorbslam_amd import MapDb
    m = MC.scene()
    T = m["table"]
    rng = np.random.default_rng(23)
    blocks = [rng.integers(0, 256, (16, 32)).astype(np.uint8) for _ in range(T.n_keyframes)]
    obs, _ = D.split_levels(T)
    views = [np.stack([o, (np.arange(len(o)) * 5 + p) % 16], axis=1).astype(I32) for p, o in enumerate(obs)]
    rows = [np.asarray(a, I32) for a in m["kf_points"]]
    plain, both = MapDb(0, 64, 8, 256), MapDb(0, 64, 8, 256)
    model = R.DescModel(T.n_points, T.n_keyframes)
    model.bad[:] = T.bad
    for db in (plain, both):
        D.load(db, m)
        db.set_keyframe_rows(np.arange(T.n_keyframes), rows)
    sf = S.scale_factors()
    q = np.arange(T.n_keyframes, dtype=I32)
    model.send(both, blocks=(q, blocks))
    a, b = plain.update_normal_depth(np.arange(T.n_points), sf), both.update_normal_depth(np.arange(T.n_points), sf)
    S.same_normal_depth(b, a)
    model.send(both, views=(np.arange(T.n_points), views))
    S.same_covisibility(both.covisibility(q, m["kf_points"]), plain.covisibility(q, m["kf_points"]))
    got = model.check_query(both, np.arange(T.n_points), oracle_lib)
    assert (got["status"] == R.UPDATED).sum() > 400 and (got["status"] == R.BAD).sum() == int(T.bad.sum())
    pa, pb = plain.points_of_keyframes([3, 1, 7], [5, 9]), both.points_of_keyframes([3, 1, 7], [5, 9])
    assert np.array_equal(pa["slots"], pb["slots"]) and np.array_equal(pa["seen"], pb["seen"])
    args = MC.shape_a(m)
    MC.same_correction(both.correct(**args), plain.correct(**args))
    model.send(both, blocks=([2, 5], [np.zeros((0, 32), np.uint8), blocks[5][:9]]))   # a keyframe culled, one re-made shorter: some views lie past it now
    S.same_normal_depth(both.update_normal_depth(np.arange(T.n_points), sf), plain.update_normal_depth(np.arange(T.n_points), sf))
    got = model.check_query(both, np.arange(T.n_points), oracle_lib)
    assert (got["status"] == R.VIEW_OUT_OF_RANGE).sum() > 10
    D.same_export(both.export(), plain.export())
    model.check_exports(both)
    plain.close()
    both.close()


def test_fuzz_against_the_oracle(oracle_lib):
    """300 points over 40 keyframes; descriptors from four base rows with a few flipped bits, so that medians collide often."""
    rng = np.random.default_rng(20240917)
    base = rng.integers(0, 256, (4, 32)).astype(np.uint8)
    db, model = _handle(300, 40, bad=range(7, 300, 29))
    model.send(db, blocks=(np.arange(38), [_near(rng, base, int(rng.integers(1, 17))) for _ in range(38)]))
    views = []
    for _ in range(300):
        k = rng.integers(0, 40, int(rng.integers(0, 25)))
        views.append(np.stack([k, [rng.integers(0, max(len(model.blocks[j]), 1)) for j in k]], axis=1).astype(I32).reshape(-1, 2))
    model.send(db, views=(np.arange(300), views))
    got = model.check_query(db, rng.permutation(300), oracle_lib)
    ties = sum(R.median_ties(np.stack([model.blocks[k][i] for k, i in model.views[p] if len(model.blocks[k])]))[1] > 1
               for p in range(300) if not model.bad[p] and any(len(model.blocks[k]) for k, _ in model.views[p]))
    assert (got["status"] == R.UPDATED).sum() > 250 and ties > 100
    db.close()
