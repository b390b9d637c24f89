"""The resident table's keyframe rows on the GPU (ydorbslam_amd/csrc/map_resident.hip, mapdb_rows_kernels.hip.h): rows loaded and
changed by deltas, the points of a keyframe set and the observer counter of point lists against the CPU restatement
(tests/localmap_ref) on the exported table, and the seeded sequence of tests/cpu_harness/mapdb_rows_check.cpp through the real handle
against that program's counters.  Every comparison is exact integer equality."""
import numpy as np
import pytest

import mapdb_rows_support as R

pytestmark = pytest.mark.gpu
I32 = np.int32


def _db(*caps):
    from ydorbslam_amd import MapDb
    return MapDb(0, *caps)


def _points(db, n, n_kf, bad=(), first=0):
    """Point slots first .. first+n-1, each observed by one or two of n_kf keyframes; `bad` = the slots flagged bad."""
    db.set_centres(np.arange(n_kf), np.zeros((n_kf, 3), np.float32))
    slots = np.arange(first, first + n)
    obs = [np.array(sorted({p % n_kf, (7 * p + 1) % n_kf}), I32) for p in slots]
    flag = np.isin(slots, list(bad)).astype(np.uint8)
    db.set_points(slots, obs, [np.zeros(len(o), np.uint8) for o in obs], flag, [o[0] for o in obs], np.zeros(n, np.uint8), np.zeros((n, 3), np.float32))


def _row(rng, n, n_points, null_share=0.25):
    r = rng.integers(0, n_points, n).astype(I32)
    r[rng.random(n) < null_share] = -1
    return r


@pytest.fixture(scope="module")
def sized():
    """One handle for the |E| cases: 1 000 points (every 11th bad), keyframe k's row has SIZES[k] entries."""
    sizes = (1, 63, 64, 65, 255, 256, 257, 3 * 256 + 1)
    db = _db(1024, 8, 4096)
    _points(db, 1000, 8, bad=range(5, 1000, 11))
    rng = np.random.default_rng(3)
    rows = [_row(rng, n, 1000, 0.1) for n in sizes]
    rows[0][0] = 17
    db.set_keyframe_rows(np.arange(8), rows)
    exported = (db.export_rows(), db.export()["table"].bad)
    R.same_rows(exported[0], rows)
    yield db, sizes, exported
    db.close()


def test_rows_loaded_in_three_shuffled_calls_equal_the_model():
    rng = np.random.default_rng(1)
    db = _db(256, 8, 1000)                                         # headers and row pool grow during the load
    _points(db, 400, 30, bad=(3, 50))
    rows = [_row(rng, int(n), 400) for n in rng.integers(0, 200, 30)]
    for part in np.array_split(rng.permutation(30), 3):
        db.set_keyframe_rows(part, [rows[k] for k in part])
    R.same_rows(db.export_rows(), rows)
    s = db.row_stats()
    assert s["n_entries"] == sum(len(r) for r in rows) and s["header_growths"] >= 1 and s["repacks_grown"] >= 1
    R.check_points_of_keyframes(db, rng.permutation(30)[:12], rng.integers(0, 400, 50))
    db.close()


def test_the_seeded_sequence_on_the_device_equals_the_model_and_the_cpu_trace(tmp_path):
    rounds = R.sequence(str(tmp_path))
    traces = [r[-1][1] for r in rounds]
    kept = next(i for i, t in enumerate(traces) if t["repacks_kept"] == 1)
    grown = next(i for i, t in enumerate(traces) if t["repacks_grown"] == 1)
    hdr = next(i for i, t in enumerate(traces) if t["header_growths"] == 1)
    db, model = _db(*R.SEQUENCE_CAPACITIES), R.RowModel()
    _points(db, R.SEQUENCE_POINTS, 4, bad=range(0, R.SEQUENCE_POINTS, 9))
    bad = db.export()["table"].bad
    base = db.stats()
    for i, ops in enumerate(rounds):
        for op in ops[:-1]:
            model.apply(op)
            model.send(db, op)
        rows = db.export_rows()                                    # export applies what is staged: the round's one sync
        R.same_rows(rows, model.rows)
        got = db.row_stats()
        assert {k: got[k] for k in R.TRACE_FIELDS[2:]} == {k: traces[i][k] for k in R.TRACE_FIELDS[2:]}, i
        st = db.stats()
        assert st["n_keyframes"] == traces[i]["n_keyframes"] and st["last_sync_bytes"] == 0   # row traffic is not in YdMapDbStats
        assert {k: st[k] for k in ("n_points", "n_observations", "pool_used", "repacks_kept", "repacks_grown")} == {k: base[k] for k in ("n_points", "n_observations", "pool_used", "repacks_kept", "repacks_grown")}
        if i in (0, grown, kept - 1, kept, hdr, len(rounds) - 1):
            R.check_points_of_keyframes(db, np.arange(len(rows))[::-1], np.arange(0, 500, 3), exported=(rows, bad))
            assert db.row_stats()["last_row_sync_bytes"] == 0      # the query found nothing staged
    db.close()


def test_repacks_move_rows_of_63_64_65_and_300_entries():
    rng = np.random.default_rng(5)
    # 492 + 2 x 100 > 600 with 592 live: grown, and two more appends follow; 492 + 4 x 400 > 2 000 with 892 <= 1 000 live: kept
    for pool, filler, want, used in ((600, 100, "repacks_grown", 792), (2000, 400, "repacks_kept", 892)):
        db = _db(512, 8, pool)
        _points(db, 500, 6)
        rows = [_row(rng, n, 500) for n in (63, 64, 65, 300)] + [np.zeros(0, I32)]
        db.set_keyframe_rows(np.arange(4), rows[:4])
        for _ in range(4):                                         # row 4 replaced until the append does not fit
            rows[4] = _row(rng, filler, 500)
            db.set_keyframe_rows([4], [rows[4]])
            R.same_rows(db.export_rows(), rows, 6)
        s = db.row_stats()
        assert s[want] == 1 and s["repacks_kept"] + s["repacks_grown"] == 1 and s["n_entries"] == 492 + filler and s["pool_used"] == used
        R.check_points_of_keyframes(db, [3, 4, 0, 1, 2])
        db.close()


def test_entry_deltas_on_a_staged_row_and_on_a_resident_row():
    db = _db(64, 4, 256)
    _points(db, 40, 3)
    db.set_keyframe_rows([0, 1], [[1, 2, 3, 4], [5, 6, 7]])
    db.set_row_entries([0, 1], [3, 0], [-1, 30])                   # the rows are staged in the same sync
    R.same_rows(db.export_rows(), [[1, 2, 3, -1], [30, 6, 7]], 3)
    assert db.row_stats()["last_row_sync_records"] == 2
    db.set_row_entries([0, 1, 0], [0, 2, 0], [11, 12, 13])          # resident rows; (0, 0) twice: the last value, one record
    R.same_rows(db.export_rows(), [[13, 2, 3, -1], [30, 6, 12]], 3)
    s = db.row_stats()
    assert s["last_row_sync_records"] == 2 and s["last_row_sync_bytes"] == 16 and s["pool_used"] == 7
    got = db.points_of_keyframes([1, 0])
    assert got["slots"].tolist() == [30, 6, 12, 13, 2, 3] and db.row_stats()["last_row_sync_bytes"] == 0
    from ydorbslam_amd import YdorbError
    with pytest.raises(YdorbError, match="outside the row of 4 entries"):
        db.set_row_entries([0], [4], [1])
    with pytest.raises(YdorbError, match="set the point before a row names it"):
        db.set_keyframe_rows([2], [[40]])
    db.close()


@pytest.mark.parametrize("k", range(8))
def test_points_of_keyframes_across_wave_and_workgroup_boundaries(sized, k):
    """|E| of 1, 63, 64, 65, 255, 256, 257 and 3 x 256 + 1.  (With k_rowset_emit's base taken without the workgroups before it, the
    257-entry case and the last one fail: checked once during development.)"""
    db, sizes, exported = sized
    got = R.check_points_of_keyframes(db, [k], exported=exported)
    assert got["count"] <= sizes[k] and (k > 0 or got["slots"].tolist() == [17])


def test_two_different_queries_back_to_back_and_the_whole_set(sized):
    db, _, exported = sized
    seen = np.array([17, -1, 900, 900, 3], I32)
    a = R.check_points_of_keyframes(db, [7, 6], seen, exported=exported)
    b = R.check_points_of_keyframes(db, [6, 7], exported=exported)    # the other order: another list, the same set
    assert sorted(a["slots"].tolist()) == sorted(b["slots"].tolist()) and a["slots"].tolist() != b["slots"].tolist() and not b["seen"].any()
    R.check_points_of_keyframes(db, np.arange(8), seen, exported=exported)
    R.check_points_of_keyframes(db, [7, 6], exported=exported)       # a first / seen scratch that was not put back would show here


def test_first_occurrence():
    db = _db(64, 4, 2048)
    _points(db, 50, 5)
    far = np.full(600, -1, I32)
    far[3], far[400], far[599] = 7, 7, 8                           # 7: first in workgroup 0, again in workgroup 1
    db.set_keyframe_rows([0, 1, 2, 4], [far, [9, 9, 4, 9], [7, 9, 20], [7, 9, 8, 21]])
    for kfs, want in (([0], [7, 8]), ([1], [9, 4]), ([2, 1, 0, 4], [7, 9, 20, 4, 8, 21]), ([1, 1], [9, 4]), ([4, 0, 4, 2], [7, 9, 8, 21, 20])):
        got = R.check_points_of_keyframes(db, kfs)
        assert got["slots"].tolist() == want, kfs
    db.close()


def test_null_rows_bad_points_empty_rows_and_never_set_slots():
    db = _db(64, 4, 512)
    _points(db, 1, 6)                                               # slot 0 ...
    _points(db, 1, 6, first=9)                                      # ... and slot 9: 1 .. 8 were never set and read as bad
    _points(db, 3, 6, bad=(10, 11, 12), first=10)
    db.set_keyframe_rows([0, 1, 2, 3], [[-1] * 70, [10, 11, 12, 11], [], [0, 5, 9, -1, 3]])
    assert db.n_keyframes == 6
    for kfs, want in (([0], []), ([1], []), ([2], []), ([5], []), ([0, 2, 5, 1], []), ([1, 2, 3, 5, 0], [0, 9]), ([3], [0, 9])):
        got = R.check_points_of_keyframes(db, kfs, [9])
        assert got["slots"].tolist() == want and got["seen"].tolist() == [1 if s == 9 else 0 for s in want]
    assert db.points_of_keyframes([])["count"] == 0
    from ydorbslam_amd import YdorbError
    with pytest.raises(YdorbError, match="keyframe slot 6 outside 0..5"):
        db.points_of_keyframes([6])
    with pytest.raises(YdorbError, match=r"seen_points\[1\]: point slot 13 outside -1..12"):
        db.points_of_keyframes([3], [0, 13])
    db.close()


def test_capacity_that_fits_exactly_and_that_misses_by_one(sized):
    db, _, exported = sized
    want, _ = R.ref_points_of_keyframes(exported[0], exported[1], [6, 2])
    fit = db.points_of_keyframes([6, 2], capacity=len(want))
    assert fit["status"] == 0 and np.array_equal(fit["slots"], want)
    miss = db.points_of_keyframes([6, 2], [int(want[0])], capacity=len(want) - 1)
    assert miss["status"] == 1 and miss["count"] == len(want) and (miss["raw_slots"] == -7).all() and (miss["raw_seen"] == 7).all()
    R.check_points_of_keyframes(db, [6, 2], [int(want[0])], exported=exported)   # the refused query left no mark behind


def test_seen_points_with_nulls_duplicates_and_points_in_no_row(sized):
    db, _, exported = sized
    in_rows = exported[0][4][exported[0][4] >= 0]
    absent = np.setdiff1d(np.arange(1000), np.concatenate(exported[0]))[:5]
    seen = np.concatenate([[-1], in_rows[:20], in_rows[:20], absent, [-1]]).astype(I32)
    got = R.check_points_of_keyframes(db, [4, 5], seen, exported=exported)
    assert got["seen"].sum() > 0
    assert not R.check_points_of_keyframes(db, [4, 5], absent, exported=exported)["seen"].any()


def test_a_query_after_a_point_table_growth_clear_and_two_handles():
    a, b = _db(32, 4, 128), _db(32, 4, 128)
    _points(a, 30, 3)
    _points(b, 20, 3, bad=(1,))
    a.set_keyframe_rows([0, 1], [[1, 2, 29, 2], [29, 5]])
    b.set_keyframe_rows([0], [[1, 2, 19]])
    assert R.check_points_of_keyframes(a, [0, 1], [29])["slots"].tolist() == [1, 2, 29, 5]
    assert R.check_points_of_keyframes(b, [0])["slots"].tolist() == [2, 19]
    _points(a, 100, 3, first=30)                                    # past the capacity of 32: the point table and the scratch grow
    a.set_row_entries([1], [1], [120])
    assert a.stats()["point_table_growths"] == 0                    # staged only
    assert R.check_points_of_keyframes(a, [1, 0], [120, 1])["slots"].tolist() == [29, 120, 1, 2] and a.stats()["point_table_growths"] == 1
    assert R.check_points_of_keyframes(a, [0], [120, 1])["slots"].tolist() == [1, 2, 29]
    a.clear()
    assert a.row_stats()["n_entries"] == 0 and a.row_stats()["pool_used"] == 0 and a.n_keyframes == 0 and a.export_rows() == []
    _points(a, 10, 2)
    a.set_keyframe_rows([1], [[3, 3, 4]])
    assert R.check_points_of_keyframes(a, [0, 1], [4])["slots"].tolist() == [3, 4]
    assert R.check_points_of_keyframes(b, [0])["slots"].tolist() == [2, 19]
    a.close()
    b.close()


def test_upload_accounting_rows_and_points_are_counted_apart():
    db = _db(64, 4, 256)
    _points(db, 20, 3)
    db.export()
    points_bytes = db.stats()["last_sync_bytes"]
    assert points_bytes > 0 and db.row_stats()["last_row_sync_bytes"] == 0
    db.set_keyframe_rows([0, 5], [[1, 2, 3], [4]])                  # names keyframe slot 5: n_keyframes grows with no centre record
    assert db.n_keyframes == 6
    db.points_of_keyframes([0])
    assert db.row_stats()["last_row_sync_bytes"] == 2 * 16 + 16 and db.stats()["last_sync_bytes"] == 0 and db.stats()["last_sync_records"] == 0
    db.points_of_keyframes([0])
    assert db.row_stats()["last_row_sync_bytes"] == 0 and db.row_stats()["last_row_sync_records"] == 0
    assert np.array_equal(db.export()["centre"], np.zeros((6, 3), np.float32))
    db.close()


def _same_counter(db, lists, table):
    got = db.observer_counter(lists)
    for q, pts in enumerate(lists):
        kf, w, pb = R.ref_observer_counter(table, pts)
        assert got["status"][q] == 0 and got["counts"][q] == len(kf)
        assert np.array_equal(got["kf"][q], kf) and np.array_equal(got["weight"][q], w) and np.array_equal(got["point_bad"][q], pb), q
    return got


def test_observer_counter_lists_nulls_repeats_and_bad_points():
    db = _db(256, 16, 1024)
    _points(db, 200, 12, bad=(4, 77))
    table = db.export()["table"]
    rng = np.random.default_rng(9)
    one = np.array([0, -1, 3, 3, 4, 77, 199, -1, 3], I32)           # 3 listed three times counts three times
    got = _same_counter(db, [one], table)
    assert got["point_bad"][0].tolist() == [0, 0, 0, 0, 1, 1, 0, 0, 0] and got["weight"][0][got["kf"][0].tolist().index(3)] >= 3
    lists = [one, np.zeros(0, I32), _row(rng, 150, 200), np.full(5, -1, I32), np.arange(200, dtype=I32)]
    _same_counter(db, lists, table)
    # against ydorb_mapdb_covisibility: its result plus the self slot's own count
    pts = np.arange(0, 200, 3, dtype=I32)
    full = db.observer_counter([pts])
    self_kf = 3                                                     # observes points 3, 15, 27, ... of the list
    cov = db.covisibility([self_kf], [pts], capacities=[12])[0]
    own = sum(int(self_kf in table.obs_kf[table.obs_start[p]:table.obs_start[p + 1]]) for p in pts if not table.bad[p])
    merged = sorted(list(zip(cov["kf"].tolist(), cov["weight"].tolist())) + ([(self_kf, own)] if own else []))
    assert own > 0 and merged == list(zip(full["kf"][0].tolist(), full["weight"][0].tolist()))
    from ydorbslam_amd import YdorbError
    with pytest.raises(YdorbError, match="list entry 1: point slot 200 outside -1..199"):
        db.observer_counter([[0, 200]])
    with pytest.raises(YdorbError, match="point slot -2"):
        db.observer_counter([[-2]])
    db.close()


def test_observer_counter_across_the_histogram_window_boundary():
    from ydorbslam_amd import COVIS_WINDOW
    n_kf = COVIS_WINDOW + 8
    db = _db(64, 64, 256)
    db.set_centres(np.arange(n_kf), np.zeros((n_kf, 3), np.float32))
    obs = [np.array([COVIS_WINDOW - 2 + (p % 5), 1], I32) for p in range(20)]   # keyframes W-2 .. W+2 and keyframe 1
    db.set_points(np.arange(20), obs, [np.zeros(2, np.uint8)] * 20, np.zeros(20, np.uint8), [1] * 20, np.zeros(20, np.uint8), np.zeros((20, 3), np.float32))
    table = db.export()["table"]
    pts = np.arange(20, dtype=I32)
    got = _same_counter(db, [pts, pts[:7]], table)
    assert got["kf"][0].tolist() == [1] + [COVIS_WINDOW - 2 + j for j in range(5)] and got["weight"][0].tolist() == [20, 4, 4, 4, 4, 4]
    fit = db.observer_counter([pts, pts[:7]], capacities=[6, 6])
    assert fit["status"].tolist() == [0, 0] and fit["kf"][0].tolist() == got["kf"][0].tolist()
    miss = db.observer_counter([pts, pts[:7]], capacities=[5, 6])
    assert miss["status"].tolist() == [1, 0] and miss["counts"].tolist() == [6, 6] and (miss["raw_kf"][:5] == -7).all() and (miss["raw_weight"][:5] == -7).all()
    assert miss["kf"][1].tolist() == got["kf"][1].tolist()
    db.close()
