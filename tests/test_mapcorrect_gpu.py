"""ydorb_mapdb_correct on the GPU (ydorbslam_amd/csrc/mapcorrect_kernels.hip.h through map_resident.hip) against the CPU restatement
tests/mapcorrect_ref/mapcorrect_ref.cpp on the same table, exactly: status bytes and float bit patterns of the results, and the whole
table read back afterwards.  The scene, transforms and call shapes are mapcorrect_support's; test_mapcorrect_cpu.py shows that the
scene tells the interleaved order from poses-first."""
import numpy as np
import pytest

import mapcorrect_support as K
import mapdb_support as D
import mapmaint_support as S

pytestmark = pytest.mark.gpu
SF = S.scale_factors()
f32 = np.float32


def _db(*caps):
    from ydorbslam_amd import MapDb
    return MapDb(0, *caps)


@pytest.fixture(scope="module")
def m():
    return K.scene()


def _loaded(m, *caps):
    db = _db(*caps) if caps else _db()
    D.load(db, m)
    return db


# ------------------------------------------------------------------------------------------------------------ 1 the three shapes
@pytest.mark.parametrize("shape", ["A", "B", "C"])
def test_each_call_shape_equals_the_restatement_and_the_table_holds_it(m, shape):
    args = K.SHAPES[shape](m)
    want, table = K.ref_correct(m, **args)
    db = _loaded(m)
    got = db.correct(**args)
    K.same_correction(got, want)
    D.same_export(db.export(), table)
    done = np.isin(want["status"], (K.DONE, K.DONE_NO_OBS))
    assert done.sum() > 100 and (~done).any() and not got["pos"][~done].any()
    assert not np.array_equal(table["pos"], m["pos"])
    if shape != "C":                                              # the table serves the next query with what it now holds
        S.same_normal_depth(db.update_normal_depth(np.arange(600), SF),
                            S.ref_update_normal_depth(table["table"], table["pos"], table["centre"], table["ref_kf"], table["ref_level"], SF))
        assert not np.array_equal(table["centre"], m["centre"])
    db.close()


def test_loop_a_then_loop_b_on_one_handle(m):
    """The two calls of one loop closure in a row: B's correctors name the points A claimed."""
    a = K.shape_a(m)
    want_a, after_a = K.ref_correct(m, **a)
    claimed = np.zeros(600, bool)
    claimed[a["slots"][np.isin(want_a["status"], (K.DONE, K.DONE_NO_OBS))]] = True
    b = K.shape_b(after_a, claimed_by_a=claimed)
    want_b, after_b = K.ref_correct(after_a, **b)
    db = _loaded(m)
    K.same_correction(db.correct(**a), want_a)
    K.same_correction(db.correct(**b), want_b)
    D.same_export(db.export(), after_b)
    db.close()


# ------------------------------------------------------------------------------------------------------------ 2 entry counts
def test_entry_counts_around_waves_and_workgroups(m):
    """n = 1 .. 257 entries of loop A's list (bad and repeated entries in it: the claimed list is shorter than n), one call after the
    other on one handle; then n = 0, which still writes the centres."""
    a = K.shape_a(m)
    db, table = _loaded(m), m
    shorter = 0
    for n in (1, 63, 64, 65, 255, 256, 257):
        args = K.with_entries(a, n)
        want, table = K.ref_correct(table, **args)
        K.same_correction(db.correct(**args), want)
        shorter += int((~np.isin(want["status"], (K.DONE, K.DONE_NO_OBS))).any())
    assert shorter >= 4
    b = K.shape_b(m)
    for n in (257, 600):                                          # by name and by null slots
        args = K.with_entries(b, n) if n < 600 else b
        want, table = K.ref_correct(table, **args)
        K.same_correction(db.correct(**args), want)
    D.same_export(db.export(), table)
    args = dict(K.with_entries(a, 0), centre_after=K.new_centres(77, m, a["kf_slots"]))
    want, table = K.ref_correct(table, **args)
    got = db.correct(**args)
    assert len(got["status"]) == 0 and len(want["status"]) == 0
    D.same_export(db.export(), table)
    assert np.array_equal(table["centre"][a["kf_slots"]], args["centre_after"])
    db.close()


# ------------------------------------------------------------------------------------------------------------ 3 the hand-built list
def _small_map():
    """5 keyframes, 8 point slots: 0 good, 1 bad, 2 never set, 3 an empty span that is not bad, 4 good, 5 good with reference keyframe 4,
    6 good, 7 good."""
    from ydorbslam_amd.map_maintenance import ObservationTable
    obs = [[0, 1, 2], [0, 1], [], [], [1, 2, 3], [4, 0], [2, 0, 3], [3]]
    lev = [[0, 1, 2], [1, 1], [], [], [2, 0, 1], [3, 3], [1, 1, 7], [4]]
    T = ObservationTable(5, [np.array(o, np.int32) for o in obs], [np.array(l, np.uint8) for l in lev], [np.zeros(len(o), np.uint8) for o in obs],
                         np.array([0, 1, 1, 0, 0, 0, 0, 0], np.uint8))
    rng = np.random.default_rng(8)
    pos = rng.uniform(-3, 3, (8, 3)).astype(f32) + f32(5)
    pos[2] = 0
    return dict(table=T, pos=pos, centre=rng.uniform(-1, 1, (5, 3)).astype(f32), ref_kf=np.array([1, 0, 0, 2, 2, 4, 0, 3], np.int32),
                ref_level=np.array([1, 1, 0, 0, 0, 3, 1, 4], np.uint8))


def _load_small(sm):
    db = _db(4, 2, 4)
    db.set_centres(np.arange(5), sm["centre"])
    obs, lev = D.split_levels(sm["table"])
    keep = [0, 1, 3, 4, 5, 6, 7]                                   # slot 2 is never set
    db.set_points(keep, [obs[p] for p in keep], [lev[p] for p in keep], sm["table"].bad[keep], sm["ref_kf"][keep], sm["ref_level"][keep], sm["pos"][keep])
    return db


def test_hand_built_list_case_by_case():
    sm = _small_map()
    before, after = K.sim3_pairs(9, 4)
    kf = np.array([2, 0, 1, 3], np.int32)
    slots = [1, 2, 3, 0, 0, 4, 7, 4, 5, 6]
    corr = [0, 0, 1, 1, 1, 1, 2, 2, -1, -1]
    args = dict(kf_slots=kf, before=before, after=after, slots=slots, corrector=corr, centre_after=K.new_centres(3, sm, kf), centres="interleaved",
                scale_factors=SF)
    want, table = K.ref_correct(sm, **args)
    db = _load_small(sm)
    got = db.correct(**args)
    assert list(got["status"]) == [K.BAD,           # a bad point
                                   K.BAD,           # a slot never set
                                   K.DONE_NO_OBS,   # an empty span that is not bad: moved, no normals
                                   K.DONE,
                                   K.CLAIMED,       # repeated inside one keyframe's list
                                   K.DONE,
                                   K.DONE,
                                   K.CLAIMED,       # repeated across keyframes: the first claimed
                                   K.NOT_COVERED,   # reference keyframe 4 is not in the call
                                   K.DONE]          # reference keyframe 0 is: rank 1
    K.same_correction(got, want)
    for i in (0, 1, 4, 7, 8):
        assert not got["pos"][i].any() and not got["normal"][i].any() and got["max_distance"][i] == 0
    assert got["pos"][2].any() and not got["normal"][2].any() and got["min_distance"][2] == 0
    assert np.array_equal(got["pos"][5], table["pos"][4]) and np.array_equal(got["pos"][3], table["pos"][0])
    for p in (1, 2, 5):
        assert np.array_equal(table["pos"][p], sm["pos"][p])      # the table is left alone
    D.same_export(db.export(), table)
    db.close()


# ------------------------------------------------------------------------------------------------------------ 4 the visibility boundary
def _normal(P, centres):
    """updateNormalAndDepth's sum over the given centres, in order, in the operations of DESIGN.md section 2."""
    acc = np.zeros(3, f32)
    for c in centres:
        d = (P - c).astype(f32)
        dd = d.astype(np.float64)
        inv = f32(1.0 / np.sqrt((dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2]))
        acc = (acc + d * inv).astype(f32)
    return acc * f32(1.0 / len(centres))


def test_visibility_boundary():
    """One point claimed at rank 1 with observers at ranks 0, 1, 2 and one outside the call: only rank 0 shows its new centre; under
    poses-first all three do; the reference keyframe's centre in the distance follows the same rule."""
    from ydorbslam_amd.map_maintenance import ObservationTable
    T = ObservationTable(5, [np.array([3, 4, 0, 2], np.int32)], [np.array([1, 0, 2, 1], np.uint8)], [np.zeros(4, np.uint8)], np.zeros(1, np.uint8))
    rng = np.random.default_rng(12)
    centre, new = rng.uniform(-2, 2, (5, 3)).astype(f32), rng.uniform(-2, 2, (3, 3)).astype(f32)
    kf = np.array([4, 0, 3], np.int32)                            # ranks: keyframe 4 -> 0, 0 -> 1, 3 -> 2; keyframe 2 is outside
    ident = np.repeat(np.array([[0, 0, 0, 1, 0, 0, 0, 1]], np.float64), 3, axis=0)
    P = np.array([1.5, 2.5, 9.0], f32)
    for rule, ref_kf, seen in (("interleaved", 4, {4: new[0]}), ("interleaved", 0, {4: new[0]}), ("poses_first", 3, {4: new[0], 0: new[1], 3: new[2]}),
                               ("resident", 4, {})):
        sm = dict(table=T, pos=P[None].copy(), centre=centre, ref_kf=np.array([ref_kf], np.int32), ref_level=np.array([1], np.uint8))
        args = dict(kf_slots=kf, before=ident, after=ident, slots=[0], corrector=[1], centre_after=new, centres=rule, scale_factors=SF)
        db = _db()
        D.load(db, sm)
        got = db.correct(**args)
        cen = lambda k: seen.get(k, centre[k])
        assert np.array_equal(got["normal"][0].view(np.uint32), _normal(P, [cen(3), cen(4), cen(0), cen(2)]).view(np.uint32)), rule
        d = (P - cen(ref_kf)).astype(np.float64)
        dist = f32(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
        assert got["max_distance"][0] == dist * SF[1] and got["min_distance"][0] == (dist * SF[1]) / SF[7], rule
        want, table = K.ref_correct(sm, **args)
        K.same_correction(got, want)
        D.same_export(db.export(), table)
        db.close()


# ------------------------------------------------------------------------------------------------------------ 5 staged changes
def test_a_staged_delta_lands_before_the_correction(m):
    db = _loaded(m)
    db.export()                                                   # the load is on the device
    rng = np.random.default_rng(21)
    model = dict(m, pos=m["pos"].copy(), ref_kf=m["ref_kf"].copy(), ref_level=m["ref_level"].copy())
    moved = rng.permutation(600)[:50]
    model["pos"][moved] = rng.uniform(-5, 5, (50, 3)).astype(f32)
    db.set_positions(moved, model["pos"][moved])
    obs, lev = D.split_levels(m["table"])
    again = [p for p in rng.permutation(600)[:60] if len(obs[p]) > 1][:20]
    for p in again:                                               # another reference keyframe among the point's observers
        model["ref_kf"][p], model["ref_level"][p] = obs[p][-1], lev[p][-1] & 0x7f
    db.set_points(again, [obs[p] for p in again], [lev[p] for p in again], m["table"].bad[again], model["ref_kf"][again], model["ref_level"][again],
                  model["pos"][again])
    args = K.shape_b(model)
    want, table = K.ref_correct(model, **args)
    K.same_correction(db.correct(**args), want)
    assert db.stats()["last_sync_records"] >= 50
    D.same_export(db.export(), table)
    db.close()


def test_corrected_positions_survive_a_repack_and_a_table_growth(m):
    from ydorbslam_amd.map_maintenance import ObservationTable, _csr
    T = m["table"]
    N = int(T.obs_start[-1])
    db = _loaded(m, 600, 40, N + 8)
    args = K.shape_a(m)
    want, table = K.ref_correct(m, **args)
    K.same_correction(db.correct(**args), want)
    before = db.stats()
    obs, lev = D.split_levels(T)
    new = np.arange(600, 900)
    rng = np.random.default_rng(4)
    new_pos = rng.uniform(-5, 5, (300, 3)).astype(f32)
    db.set_points(new, obs[:300], lev[:300], T.bad[:300], m["ref_kf"][:300], m["ref_level"][:300], new_pos)
    start, kf = _csr(obs + obs[:300], np.int32)
    _, lv = _csr(lev + lev[:300], np.uint8)
    grown = dict(table=ObservationTable.from_arrays(40, start, kf, lv, np.concatenate([T.bad, T.bad[:300]])),
                 pos=np.concatenate([table["pos"], new_pos]), centre=table["centre"], ref_kf=np.concatenate([m["ref_kf"], m["ref_kf"][:300]]),
                 ref_level=np.concatenate([m["ref_level"], m["ref_level"][:300]]))
    D.same_export(db.export(), grown)
    s = db.stats()
    assert s["point_table_growths"] == before["point_table_growths"] + 1
    assert s["repacks_kept"] + s["repacks_grown"] == before["repacks_kept"] + before["repacks_grown"] + 1
    args = K.shape_c(grown)                                       # and the next correction works on the grown table
    want, table = K.ref_correct(grown, **args)
    K.same_correction(db.correct(**args), want)
    D.same_export(db.export(), table)
    db.close()


# ------------------------------------------------------------------------------------------------------------ 6 repeatability, isolation
def test_two_handles_give_identical_bytes_and_a_refused_call_changes_nothing(m):
    from ydorbslam_amd import YdorbError
    a, c = K.shape_a(m), K.shape_c(m)
    outs, exports = [], []
    for _ in range(2):
        db = _loaded(m)
        outs.append((db.correct(**a), db.correct(**c)))
        exports.append(db.export())
    for x, y in zip(outs[0], outs[1]):
        K.same_correction(x, y)
    D.same_export(exports[0], exports[1])
    held = exports[1]
    db.set_positions([3], np.ones((1, 3), f32))                   # staged: a refused call must not apply it either
    staged = db.stats()
    for bad_args, text in ((dict(a, kf_slots=np.concatenate([a["kf_slots"][:-1], a["kf_slots"][:1]])), "repeats kf_slots"),
                           (dict(a, slots=np.concatenate([a["slots"][:-1], [600]]).astype(np.int32)), "point slot 600 outside 0..599"),
                           (dict(a, corrector=np.full(len(a["slots"]), 14, np.int32)), "outside -1..13"),
                           (dict(a, centre_after=None), "without centre_after"),
                           (dict(a, scale_factors=np.ones(9, f32)), "n_levels 9"),
                           (dict(a, scale_factors=SF[:3]), ">= n_levels"),
                           (dict(a, after=np.where(np.arange(8) == 7, 0.0, a["after"])), "Sim3 scale"),
                           (dict(c, arithmetic="sim3", before=np.ones((30, 8)), after=np.ones((30, 8)), centres="poses_first"), "without centre_after")):
        with pytest.raises(YdorbError, match=text):
            db.correct(**bad_args)
    assert db.stats() == staged
    held["pos"][3] = 1
    D.same_export(db.export(), held)
    db.close()


# ------------------------------------------------------------------------------------------------------------ 7 upload accounting
def test_nothing_staged_no_table_byte_moves(m):
    db = _loaded(m)
    db.export()
    for shape in ("A", "C"):
        db.correct(**K.SHAPES[shape](m))
        s = db.stats()
        assert s["last_sync_bytes"] == 0 and s["last_sync_records"] == 0
    db.close()
