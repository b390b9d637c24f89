"""The resident table's point attributes on the GPU (ydorbslam_amd/csrc/map_resident.hip, mapdb_attr_kernels.hip.h): the seeded sequence
of tests/cpu_harness/mapdb_attr_check.cpp replayed through the real handle against the naive model and that program's counters, a
handle that never enables the relation against one that does, and the write-through of the three queries that compute what the relation
holds.  Every comparison is exact.  At most 600 points and 40 keyframes."""
import numpy as np
import pytest

import frustum_support as F
import mapcorrect_support as MC
import mapdb_attr_support as R
import mapdb_desc_support as DS
import mapdb_support as D
import mapmaint_support as S

pytestmark = pytest.mark.gpu
I32 = np.int32


def _db(caps=(1024, 64, 8192), attributes=True):
    from ydorbslam_amd import MapDb
    db = MapDb(0, *caps)
    if attributes:
        db.enable_attributes()
    return db


def _all_stats(db):
    return db.stats(), db.row_stats(), db.desc_stats()


def test_the_seeded_sequence_equals_the_model_and_the_counters(tmp_path):
    rounds = R.sequence(str(tmp_path))
    assert len(rounds) == 40
    db, plain, model = _db(R.SEQUENCE_CAPACITIES), _db(R.SEQUENCE_CAPACITIES, attributes=False), R.AttrModel()
    for h in (db, plain):
        h.set_centres([0], np.zeros((1, 3), np.float32))
    for ops in rounds:
        for op in ops:
            if op[0] == "P":
                _, slots, bad = op
                n = len(slots)
                pos = np.zeros((n, 3), np.float32)
                pos[:, 0] = slots
                for h in (db, plain):
                    h.set_points(slots, [np.zeros(0 if b else 1, I32) for b in bad], [np.zeros(0 if b else 1, np.uint8) for b in bad], bad, np.zeros(n, I32),
                                 np.zeros(n, np.uint8), pos)
                model.set_points(slots, bad)
            elif op[0] == "A":
                _, slots, _groups, geo, desc = op
                g = (None, None, None) if geo is None else (geo[:, :3], geo[:, 3], geo[:, 4])
                db.set_point_attributes(slots, g[0], g[1], g[2], desc)
                model.set(slots, g[0], g[1], g[2], desc)
            else:
                trace = op[1]
                model.grow(trace["n_points"])
                model.check_export(db)
                got = db.attr_stats()
                assert {k: got[k] for k in R.TRACE_FIELDS[1:6]} == {k: trace[k] for k in R.TRACE_FIELDS[1:6]}, trace["round"]
                assert got["last_write_through_records"] == 0 and db.n_points == trace["n_points"]
                plain.export()
                assert _all_stats(db) == _all_stats(plain)               # the other three stats structs do not move
    assert db.attr_stats()["growths"] == 2
    db.clear()
    assert not any(a.any() for a in db.export_attributes().values()) and db.attr_stats()["capacity"] == 256
    db.close()
    plain.close()


@pytest.fixture(scope="module")
def world():
    """MC.scene() in two handles, one with attributes; 12 keyframes hold descriptor blocks and every third point has views in them."""
    m = MC.scene()
    rng = np.random.default_rng(23)
    T = m["table"]
    blocks = [rng.integers(0, 256, (16, 32)).astype(np.uint8) for _ in range(12)]
    viewed = np.arange(0, T.n_points, 3, dtype=I32)
    views = [np.stack([rng.integers(0, 14, k), rng.integers(0, 16, k)], axis=1).astype(I32) for k in rng.integers(0, 7, len(viewed))]   # keyframes 12, 13: no block
    dbs = []
    for attributes in (True, False):
        db = _db(attributes=attributes)
        D.load(db, m)
        db.set_keyframe_descriptors(np.arange(12), blocks)
        db.set_point_views(viewed, views)
        dbs.append(db)
    yield m, dbs[0], dbs[1], viewed
    for db in dbs:
        db.close()


def _sentinel(db, n, seed):
    """Stages (and does not sync) a value for every slot; returns it as a model."""
    rng = np.random.default_rng(seed)
    model = R.AttrModel()
    model.grow(n)
    v = dict(normal=rng.uniform(-1, 1, (n, 3)).astype(np.float32), mn=rng.uniform(1, 2, n).astype(np.float32), mx=rng.uniform(5, 9, n).astype(np.float32),
             desc=rng.integers(0, 256, (n, 32)).astype(np.uint8))
    db.set_point_attributes(np.arange(n), v["normal"], v["mn"], v["mx"], v["desc"])
    model.set(np.arange(n), v["normal"], v["mn"], v["mx"], v["desc"])
    return model


def test_a_handle_without_attributes_answers_the_same_and_refuses_the_new_entries(world):
    import ydorbslam_amd as y
    m, db, plain, viewed = world
    n = m["table"].n_points
    sf = S.scale_factors()
    slots = np.concatenate([np.arange(n), [5, 5, 17]]).astype(I32)
    S.same_normal_depth(db.update_normal_depth(slots, sf), plain.update_normal_depth(slots, sf))
    a, b = db.distinctive_descriptors(viewed), plain.distinctive_descriptors(viewed)
    assert all(np.array_equal(a[k], b[k]) for k in a) and sorted(set(a["status"].tolist())) == [DS.UPDATED, DS.BAD, DS.NO_DESCRIPTORS]
    assert _all_stats(db) == _all_stats(plain)
    assert plain.attr_stats() == dict(enabled=0, growths=0, capacity=0, last_attr_sync_bytes=0, last_attr_sync_records=0, last_write_through_records=0)
    one = np.zeros(1, I32)
    v, _ = F.view(*F.pose())
    with pytest.raises(y._lib.YdorbError, match="not enabled"):
        plain.set_point_attributes(one, desc=np.zeros((1, 32), np.uint8))
    with pytest.raises(y._lib.YdorbError, match="not enabled"):
        plain.export_attributes()
    with pytest.raises(y._lib.YdorbError, match="not enabled"):
        plain.frustum_cull([v], [one], [np.zeros(1, np.uint8)])
    matcher = y.OrbMatcher(0.8, check_orientation=False)
    frame = y.FrameView(np.zeros(0, y.KP_DTYPE), np.zeros((0, 32), np.uint8), (0.0, 640.0, 0.0, 480.0), None)
    with pytest.raises(y._lib.YdorbError, match="not enabled"):
        plain.search_local_points(matcher, frame, v, one, np.zeros(1, np.uint8), 3.0)
    with pytest.raises(y._lib.YdorbError, match=r"point_slots\[0\]: point slot 600 outside 0..599"):
        db.search_local_points(matcher, frame, v, [n], np.zeros(1, np.uint8), 3.0)
    matcher.close()
    assert _all_stats(db) == _all_stats(plain)


def test_update_normal_depth_writes_through(world):
    m, db, _plain, _ = world
    n = m["table"].n_points
    model = _sentinel(db, n, 1)
    slots = np.concatenate([np.arange(0, n, 2), [4, 4, 10]]).astype(I32)       # every second slot, three of them again
    got = db.update_normal_depth(slots, S.scale_factors())
    done = got["status"] == 0
    assert done.any() and (~done).any() and db.attr_stats()["last_write_through_records"] == int(done.sum())
    assert db.attr_stats()["last_attr_sync_records"] == n                    # the staged setter went first, and lost
    model.set(slots[done], got["normal"][done], got["min_distance"][done], got["max_distance"][done])
    model.check_export(db)


def test_correct_with_normals_writes_the_done_entries_through_and_without_normals_nothing():
    m = MC.scene()
    db, plain = _db(), _db(attributes=False)
    D.load(db, m)
    D.load(plain, m)
    n = m["table"].n_points
    model = _sentinel(db, n, 2)
    args = MC.shape_a(m)                                                       # SIM3, INTERLEAVED, normals
    got = db.correct(**args)
    MC.same_correction(got, plain.correct(**args))
    st = got["status"]
    assert set(st.tolist()) >= {0, 1, 2} and db.attr_stats()["last_write_through_records"] == int((st == 0).sum())
    done = st == 0
    model.set(args["slots"][done], got["normal"][done], got["min_distance"][done], got["max_distance"][done])
    before = model.check_export(db)
    c = MC.shape_c(m)                                                          # SE3, no normals pass
    got = db.correct(**c)
    MC.same_correction(got, plain.correct(**c))
    assert _all_stats(db) == _all_stats(plain)
    plain.close()
    assert (got["status"] == 0).any() and db.attr_stats()["last_write_through_records"] == 0
    after = db.export_attributes()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    db.close()


def test_distinctive_descriptors_write_through(world):
    m, db, _plain, viewed = world
    n = m["table"].n_points
    model = _sentinel(db, n, 3)
    slots = np.concatenate([viewed, viewed[:3]])
    got = db.distinctive_descriptors(slots)
    done = got["status"] == DS.UPDATED
    assert done.any() and (~done).any() and db.attr_stats()["last_write_through_records"] == int(done.sum())
    model.set(slots[done], desc=got["desc"][done])
    model.check_export(db)


# ------------------------------------------------------------------------------------------------------------ frustum test and fused search
LENGTHS = (0, 1, 63, 64, 65, 257)          # one lane per entry in blocks of 256: none, one, around a wave, more than one block
TH, RATIO = 3.0, 0.8


class Resident:
    """A frustum_support PointTable loaded into a handle at shuffled, non-contiguous slots, and the test's own copy of every value (the
    truth): the references are built from the truth, never from what the handle returns.  has_obs[i] decides the span (one observation or
    none), bad[i] the resident bad flag."""

    def __init__(self, table, has_obs, bad, seed, universe=400, capacity=512):
        rng = np.random.default_rng(seed)
        self.n = table.n
        self.slot = rng.permutation(universe)[:self.n].astype(I32)
        self.pos, self.normal = table.pos_min[:, :3].copy(), table.normal_max[:, :3].copy()
        self.mx = table.max_distance.copy()
        self.mn = (self.mx / F.scale_factors()[7]).astype(np.float32)      # the raw minimum distance the scenes derive theirs from
        # a precondition of the fixture, not a test of the feature: the truth's 0.8f * min and 1.2f * max are the bits the scene's own
        # table carries, so the references below test the same numbers
        assert np.array_equal(R.bits(np.float32(0.8) * self.mn), R.bits(table.pos_min[:, 3]))
        assert np.array_equal(R.bits(np.float32(1.2) * self.mx), R.bits(table.normal_max[:, 3]))
        self.desc = np.zeros((self.n, 32), np.uint8) if table.desc is None else table.desc.copy()
        self.has_obs, self.bad = np.asarray(has_obs, np.uint8).copy(), np.asarray(bad, np.uint8).copy()
        self.db = _db((capacity, 4, 1024))
        self.db.set_centres([0], np.zeros((1, 3), np.float32))
        self.set_points(np.arange(self.n))
        self.db.set_point_attributes(self.slot, self.normal, self.mn, self.mx, self.desc)
        self.db.export_attributes()                                        # applied: the tests start with nothing staged

    def set_points(self, idx):
        k = len(idx)
        self.db.set_points(self.slot[idx], [np.zeros(1 if h else 0, I32) for h in self.has_obs[idx]], [np.zeros(1 if h else 0, np.uint8) for h in self.has_obs[idx]],
                           self.bad[idx], np.zeros(k, I32), np.zeros(k, np.uint8), self.pos[idx])

    def table(self, idx):
        from ydorbslam_amd.frustum import PointTable
        return PointTable(self.pos[idx], self.normal[idx], np.float32(0.8) * self.mn[idx], np.float32(1.2) * self.mx[idx], self.mx[idx], self.desc[idx])


@pytest.fixture(scope="module")
def cull_scene():
    views, logs, table, _lists, _skips = F.scene()
    rng = np.random.default_rng(2)
    r = Resident(table, rng.uniform(size=table.n) < 0.8, rng.uniform(size=table.n) < 0.05, seed=4)
    yield views, logs, r
    r.db.close()


@pytest.mark.parametrize("length", LENGTHS)
def test_frustum_cull_equals_the_restatement_on_the_gathered_table(cull_scene, length):
    views, logs, r = cull_scene
    rng = np.random.default_rng(100 + length)
    lists = [rng.permutation(r.n)[:length], rng.integers(0, r.n, length), rng.permutation(r.n)[:65]]     # the second repeats slots
    skips = [(rng.uniform(size=len(a)) < 0.06).astype(np.uint8) for a in lists]
    got = r.db.frustum_cull(views, [r.slot[a] for a in lists], skips)
    assert r.db.attr_stats()["last_attr_sync_bytes"] == 0 and r.db.stats()["last_sync_bytes"] == 0        # no map byte moved
    want = F.ref_cull(views, logs, r.table(np.arange(r.n)), lists, [s | r.bad[a] for s, a in zip(skips, lists)])
    for g, w in zip(got, want):
        F.same_rows(g, w)
        assert g["n_in_view"] == w["n_in_view"]
    assert len(got[0]["status"]) == length and want[2]["n_in_view"] > 0
    # ... and on the table gathered from the handle's own exports, through the flat entry
    from ydorbslam_amd.frustum import frustum_cull
    table, _has, bad, flags = R.gathered_table(r.db, r.slot)
    assert (flags == 3).all() and np.array_equal(bad, r.bad)
    for g, w in zip(got, frustum_cull(views, table, lists, [s | r.bad[a] for s, a in zip(skips, lists)])):
        F.same_rows(g, w)


def test_frustum_cull_one_case_per_status_code():
    from ydorbslam_amd.frustum import PointTable
    views, logs, hand, lists, skips, names = F.hand_batch()
    rows = F.hand_rows()
    raw_min = np.array([rows[k]["min"] / 0.8 for k in names], np.float32)
    t = PointTable(hand.pos_min[:, :3], hand.normal_max[:, :3], np.float32(0.8) * raw_min, np.float32(1.2) * hand.max_distance, hand.max_distance)
    n = t.n
    db = _db((64, 4, 64))
    db.set_centres([0], np.zeros((1, 3), np.float32))
    slots = (3 * np.arange(n) + 1).astype(I32)
    extra = np.array([3 * n + 1, 3 * n + 4, 3 * n + 7], I32)                   # a bad point, a point without geometry, and (3 n + 2) a slot never set
    every = np.concatenate([slots, extra])
    k = len(every)
    pos = np.concatenate([t.pos_min[:, :3], np.tile(t.pos_min[names.index("in_view"), :3], (3, 1))])
    db.set_points(every, [np.zeros(1, I32)] * k, [np.zeros(1, np.uint8)] * k, np.isin(every, extra[:1]).astype(np.uint8), np.zeros(k, I32), np.zeros(k, np.uint8), pos)
    db.set_point_attributes(slots, t.normal_max[:, :3], raw_min, t.max_distance)
    iv = names.index("in_view")
    db.set_point_attributes(extra[:1], t.normal_max[iv:iv + 1, :3], raw_min[iv:iv + 1], t.max_distance[iv:iv + 1])
    db.set_point_attributes(extra[1:2], desc=np.ones((1, 32), np.uint8))       # the descriptor alone: the geometry flag stays clear
    got = db.frustum_cull(views, [[s] for s in slots], skips)
    want = F.ref_cull(views, logs, t, lists, skips)
    for name, g, w in zip(names, got, want):
        F.same_rows(g, w)
        assert g["status"][0] == rows[name]["status"], name
    assert sorted(set(int(g["status"][0]) for g in got)) == [0, 1, 2, 3, 4, 5, 6]
    v = views[iv]
    got = db.frustum_cull([v], [[extra[0], 3 * n + 2, extra[1], slots[iv]]], [np.zeros(4, np.uint8)])[0]
    assert got["status"].tolist() == [1, 1, R.NO_ATTRIBUTES, 0] and got["n_in_view"] == 1
    assert not got["rows"][:3].tobytes().strip(b"\0")
    db.close()


@pytest.fixture(scope="module")
def local():
    """frustum_support.local_map (500 keypoints, 300 map points) resident at shuffled slots: has_observations becomes the span, half of
    the skip-flagged points are resident-bad instead of flagged by the caller."""
    import ydorbslam_amd as y
    s = F.local_map()
    assert len(s["kps"]) == 500 and s["table"].n == 300
    rng = np.random.default_rng(6)
    bad = s["skip"] & (rng.uniform(size=300) < 0.5).astype(np.uint8)
    r = Resident(s["table"], s["has_obs"], bad, seed=8)
    m = y.OrbMatcher(RATIO, check_orientation=False)
    yield s, r, s["skip"] & ~bad & 1, m
    m.close()
    r.db.close()


def _frame(s, n=None):
    import ydorbslam_amd as y
    n = len(s["kps"]) if n is None else n
    return y.FrameView(s["kps"][:n], s["desc"][:n], F.BOUNDS, s["right_x"][:n])


def _same_search(got, want):
    assert got["n_to_match"] == want["n_to_match"] and got["n_matches"] == want["n_matches"]
    assert np.array_equal(got["assigned"], want["assigned"]) and np.array_equal(got["taken"], want["taken"])
    F.same_rows(got, want)


def _references(s, r, matcher, idx, skip, taken=None, assigned=None, no_attributes=()):
    """(a) ydorb_search_local_points on the table gathered in numpy from the handle's exports, (b) the restatement + matcher oracle on the
    truth.  Both see the effective skip; the entries of no_attributes are skipped there and reported as status 7 here."""
    from ydorbslam_amd.frustum import search_local_points
    eff = (np.asarray(skip, np.uint8) | r.bad[idx]).astype(np.uint8)
    eff[list(no_attributes)] = 1
    sub = dict(s, table=r.table(idx), skip=eff, has_obs=r.has_obs[idx])
    b = F.ref_search_local_points(sub, TH, RATIO, taken=taken, assigned=assigned)
    table, has, bad, _flags = R.gathered_table(r.db, r.slot[idx])
    assert np.array_equal(has, r.has_obs[idx]) and np.array_equal(bad, r.bad[idx])
    a = search_local_points(matcher, _frame(s), s["view"], table, eff, has, TH, s["taken"] if taken is None else taken, assigned)
    for w in (a, b):
        w["status"] = w["status"].copy()
        w["status"][list(no_attributes)] = R.NO_ATTRIBUTES
    return a, b


@pytest.mark.parametrize("length", LENGTHS)
def test_search_local_points_equals_both_references(local, length):
    s, r, skip, m = local
    rng = np.random.default_rng(200 + length)
    idx = rng.permutation(r.n)[:length]
    got = r.db.search_local_points(m, _frame(s), s["view"], r.slot[idx], skip[idx], TH, s["taken"])
    if length:                                                              # an empty list syncs nothing: the counters keep the fixture's sync
        assert r.db.attr_stats()["last_attr_sync_bytes"] == 0 and r.db.stats()["last_sync_bytes"] == 0    # no map byte moved
    a, b = _references(s, r, m, idx, skip[idx])
    _same_search(got, a)
    _same_search(got, b)
    if length == 257:
        assert b["n_matches"] >= 30 and b["n_to_match"] > b["n_matches"] and (got["assigned"].max() < 257)
        assert np.any((r.bad[idx] != 0) & (skip[idx] == 0)) and np.all(got["status"][r.bad[idx] != 0] == 1)   # skipped by the resident flag alone


def test_search_local_points_whole_map_repeats_and_preset_assignment(local):
    s, r, skip, m = local
    idx = np.concatenate([np.arange(r.n), [7, 7, 150, 7]])                   # slots repeated: equal rows, as the flat entry sees them
    rng = np.random.default_rng(9)
    taken = (rng.uniform(size=500) < 0.1).astype(np.uint8)
    assigned = np.where(taken != 0, 1000 + np.arange(500), -1).astype(I32)
    got = r.db.search_local_points(m, _frame(s), s["view"], r.slot[idx], skip[idx], TH, taken, assigned)
    a, b = _references(s, r, m, idx, skip[idx], taken, assigned)
    _same_search(got, a)
    _same_search(got, b)
    assert b["n_matches"] >= 30 and np.array_equal(got["assigned"][taken != 0], assigned[taken != 0])


def test_search_local_points_edges(local):
    s, r, skip, m = local
    idx = np.arange(r.n)
    # a frame with no keypoints: rows and status as ever, nothing matched
    got = r.db.search_local_points(m, _frame(s, 0), s["view"], r.slot, skip, TH)
    _, b = _references(s, r, m, idx, skip)
    F.same_rows(got, b)
    assert got["n_matches"] == 0 and got["n_to_match"] == b["n_to_match"] and len(got["assigned"]) == 0
    # no point in view: assigned untouched
    before = np.arange(500, dtype=I32) - 7
    got = r.db.search_local_points(m, _frame(s), s["view"], r.slot, np.ones(r.n, np.uint8), TH, s["taken"], before)
    assert got["n_to_match"] == 0 and got["n_matches"] == 0 and np.all(got["status"] == 1)
    assert np.array_equal(got["assigned"], before) and np.array_equal(got["taken"], s["taken"]) and not got["rows"].tobytes().strip(b"\0")
    # n == 0
    got = r.db.search_local_points(m, _frame(s), s["view"], np.zeros(0, I32), np.zeros(0, np.uint8), TH, s["taken"], before)
    assert got["n_to_match"] == 0 and got["n_matches"] == 0 and np.array_equal(got["assigned"], before)


def test_search_local_points_staged_attributes_status_7_and_growth(local):
    s, r, skip, m = local
    _, full = _references(s, r, m, np.arange(r.n), skip)
    matched = np.nonzero(full["assigned"] >= 0)[0]
    victim = int(full["assigned"][matched[0]])                               # a point the full search matches
    # staged and unsynced: the victim is erased and set again with its geometry alone; another matched point gets a new descriptor
    other = int(full["assigned"][matched[1]])
    saved = r.has_obs[victim]
    r.bad[victim], r.has_obs[victim] = 1, 0
    r.set_points(np.array([victim]))                                         # erased: bad with an empty span
    r.bad[victim], r.has_obs[victim] = 0, saved
    r.set_points(np.array([victim]))                                         # ... and the slot reused for a live point
    r.db.set_point_attributes(r.slot[[victim]], r.normal[[victim]], r.mn[[victim]], r.mx[[victim]])
    r.desc[other] = s["desc"][0]
    r.db.set_point_attributes(r.slot[[other]], desc=r.desc[[other]])
    assert r.db.attr_stats()["last_attr_sync_records"] == 0
    got = r.db.search_local_points(m, _frame(s), s["view"], r.slot, skip, TH, s["taken"])
    assert r.db.attr_stats()["last_attr_sync_records"] == 2                  # applied by the call itself
    a, b = _references(s, r, m, np.arange(r.n), skip, no_attributes=[victim])
    _same_search(got, a)
    _same_search(got, b)
    assert got["status"][victim] == R.NO_ATTRIBUTES and victim not in got["assigned"].tolist() and not got["rows"][victim:victim + 1].tobytes().strip(b"\0")
    flags = r.db.export_attributes()["flags"]
    assert flags[r.slot[victim]] == R.GEOMETRY
    # the victim gets its descriptor back, then the point table grows between two searches
    r.db.set_point_attributes(r.slot[[victim]], desc=r.desc[[victim]])
    cap = r.db.stats()["point_capacity"]
    new = np.arange(40)
    new_slots = (cap + 10 + 2 * new).astype(I32)                             # copies of the first 40 points at slots past the capacity
    r.slot = np.concatenate([r.slot, new_slots])
    for k in ("pos", "normal", "mn", "mx", "desc", "has_obs", "bad"):
        setattr(r, k, np.concatenate([getattr(r, k), getattr(r, k)[new]]))
    grown = np.arange(r.n, r.n + 40)
    r.set_points(grown)
    r.db.set_point_attributes(r.slot[grown], r.normal[grown], r.mn[grown], r.mx[grown], r.desc[grown])
    idx = np.concatenate([np.arange(100, r.n), grown])
    sk = np.concatenate([skip, skip[new]])
    got = r.db.search_local_points(m, _frame(s), s["view"], r.slot[idx], sk[idx], TH, s["taken"])
    st = r.db.attr_stats()
    assert r.db.stats()["point_capacity"] > cap and st["capacity"] == r.db.stats()["point_capacity"] and st["growths"] == 1
    a, b = _references(s, r, m, idx, sk[idx])
    _same_search(got, a)
    _same_search(got, b)
    assert (got["assigned"] >= 200).any()                                    # matches among the points past the old capacity
