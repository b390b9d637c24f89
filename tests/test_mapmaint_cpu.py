"""Map maintenance without a GPU: the CPU restatement (tests/mapmaint_ref/mapmaint_ref.cpp) against hand-computed cases, the masked
culling form against the routine that really erases, the boundaries of the culling rule, why the ABI takes the observers' order, the
host validation of the product entries and the sanitized stand-alone check of ydorbslam_amd/csrc/map_table.h.  Every comparison is
exact."""
import os
import subprocess

import numpy as np
import pytest

import mapmaint_support as S
from mapmaint_support import ROOT, f32

CHECK_SRC = os.path.join(ROOT, "tests", "cpu_harness", "map_table_check.cpp")


def _table(n_kf, observers, levels=None, stereo=None, bad=None):
    from ydorbslam_amd.map_maintenance import ObservationTable
    levels = levels if levels is not None else [[0] * len(o) for o in observers]
    return ObservationTable(n_kf, observers, levels, stereo, bad)


def test_normal_and_depth_of_a_point_with_observers_on_the_axes():
    """P = (0, 0, 0); cameras at (-2, 0, 0), (0, -4, 0), (0, 0, -8): the unit vectors are the axes, each exactly (powers of two), so
    normal = (1, 1, 1) * (float)(1.0 / 3.0).  The reference keyframe is the third at octave 2 of the pyramid 1, 2, 4, 8: dist = 8, max =
    8 * 4 = 32, min = 32 / 8 = 4.  A bad point and a point without observers give status 1 / 2 and zeros."""
    T = _table(3, [[0, 1, 2], [0, 1], []], bad=[0, 1, 0])
    centre = np.array([[-2, 0, 0], [0, -4, 0], [0, 0, -8]], f32)
    r = S.ref_update_normal_depth(T, np.zeros((3, 3), f32), centre, [2, 0, 0], [2, 0, 0], [1, 2, 4, 8])
    third = f32(1.0 / 3.0)
    assert list(r["status"]) == [0, 1, 2]
    assert np.array_equal(r["normal"][0].view(np.uint32), np.array([third] * 3, f32).view(np.uint32))
    assert r["max_distance"][0] == 32.0 and r["min_distance"][0] == 4.0
    assert not r["normal"][1:].any() and not r["max_distance"][1:].any() and not r["min_distance"][1:].any()


def test_a_point_on_an_observers_centre_gives_nan_as_the_reference_does():
    T = _table(2, [[0, 1]])
    r = S.ref_update_normal_depth(T, [[1, 2, 3]], [[1, 2, 3], [0, 0, 0]], [1], [0], [1.0])
    assert r["status"][0] == 0 and np.isnan(r["normal"][0]).all()          # 0 * inf in every component
    assert r["max_distance"][0] == r["min_distance"][0] == f32(np.sqrt(14.0))


def test_covisibility_counts_equal_bincount():
    m = S.random_map(21, 40, 600, 1, 12, bad_share=0.1)
    T, q = m["table"], np.arange(40, dtype=np.int32)
    got = S.ref_covisibility(T, q, m["kf_points"])
    for k in range(40):
        obs = [T.obs_kf[T.obs_start[p]:T.obs_start[p + 1]] for p in m["kf_points"][k] if not T.bad[p]]
        c = np.bincount(np.concatenate(obs + [np.zeros(0, np.int32)]), minlength=40)
        c[k] = 0
        assert np.array_equal(got[k]["kf"], np.nonzero(c)[0]) and np.array_equal(got[k]["weight"], c[c > 0]) and got[k]["status"] == 0
        assert got[k]["count"] == int((c > 0).sum()) <= len(got[k]["raw_kf"])          # the tight capacity holds it


def test_covisibility_counts_per_entry_and_reports_a_short_capacity():
    T = _table(5, [[0, 1, 2], [0, 2, 4], [3]], bad=[0, 0, 1])
    r = S.ref_covisibility(T, [0, 0], [[0, 1, 1, 2], [0, 1]], capacities=[3, 2])
    assert list(r[0]["kf"]) == [1, 2, 4] and list(r[0]["weight"]) == [1, 3, 2]          # point 1 is listed twice, point 2 is bad
    assert r[1]["status"] == 1 and r[1]["count"] == 3 and list(r[1]["raw_kf"]) == [-1, -1]   # nothing written


def test_redundancy_on_a_six_point_table_worked_out_by_hand():
    """Keyframes 0 .. 5; candidate 1 lists the six points with the own levels 2, 2, 0, 3, 1, 2 (thObs = 3).
         p0  observers 1 2 3 4 mono, levels 2 2 3 1: weight 4 > 3; others 2, 3, 1 <= 3 -> three -> redundant
         p1  observers 1 2 3 mono:                   weight 3, not > 3 -> counted only
         p2  observers 1 2 3 4, levels 0 1 2 1:      weight 4; others <= 1: 2 (level 1), 4 (level 1) -> two -> counted only
         p3  bad                                     -> not counted
         p4  observers 1s 2s (stereo), levels 1 5:   weight 4 > 3; others <= 2: none -> counted only
         p5  observers 2 3 4 5 1, levels 0 0 0 0 2:  weight 5; others all level 0 -> redundant (the early break stops at three)
       n_counted = 5, n_redundant = 2; 2 > 4.5 is false.  With keyframe 4 removed: p0 weight 3 -> counted only; p2 weight 3; p5 weight 4,
       others 2 3 5 -> redundant: n_counted = 5, n_redundant = 1.  With 2 and 3 removed as well: p1 has weight 1 and lost observers ->
       skipped; p0 weight 1 -> skipped; p2 weight 1 -> skipped; p4 lost keyframe 2, weight 2 -> skipped; p5 weight 2 -> skipped: 0 of 0."""
    obs = [[1, 2, 3, 4], [1, 2, 3], [1, 2, 3, 4], [1, 2], [1, 2], [2, 3, 4, 5, 1]]
    lev = [[2, 2, 3, 1], [2, 2, 2], [0, 1, 2, 1], [0, 0], [1, 5], [0, 0, 0, 0, 2]]
    st = [[0] * 4, [0] * 3, [0] * 4, [0] * 2, [1, 1], [0] * 5]
    T = _table(6, obs, lev, st, bad=[0, 0, 0, 1, 0, 0])
    args = (T, [1], [np.arange(6)], [[2, 2, 0, 3, 1, 2]])
    r = S.ref_keyframe_redundancy(*args)
    assert (r["n_counted"][0], r["n_redundant"][0], r["cull"][0]) == (5, 2, 0)
    r = S.ref_keyframe_redundancy(*args, removed=[0, 0, 0, 0, 1, 0])
    assert (r["n_counted"][0], r["n_redundant"][0], r["cull"][0]) == (5, 1, 0)
    r = S.ref_keyframe_redundancy(*args, removed=[0, 0, 1, 1, 1, 0])
    assert (r["n_counted"][0], r["n_redundant"][0], r["cull"][0]) == (0, 0, 0)


def test_redundancy_boundaries():
    """Weight exactly 3 against 4, an observer at own + 1 against own + 2, one stereo observation (weight 2, not bad: counted), 9 of 10
    (not culled) and 10 of 10 (culled): mapmaint_support.boundary_table lists each row."""
    table, cand, lists, own, want = S.boundary_table()
    r = S.ref_keyframe_redundancy(table, cand, lists, own)
    assert list(r["n_counted"]) == want["n_counted"] and list(r["n_redundant"]) == want["n_redundant"] and list(r["cull"]) == want["cull"]


@pytest.mark.parametrize("seed", S.CULLING_SEEDS)
def test_masked_form_equals_sequential_erasure(seed):
    """40 keyframes, 600 points, 1-12 observers, half stereo.  The walk that masks culled keyframes and asks again judges every candidate
    by the same two counts as the routine that erases for real, culls the same ones, and the points it skips as lost are the ones that
    routine turned bad.  At least two candidates are culled and at least one point turns bad through an erasure."""
    m = S.culling_map(seed)
    T = m["table"]
    cand, lists, own = S.candidates(m)
    seq = S.ref_sequential_culling(T, cand, lists, own)
    msk = S.masked_culling(S.ref_keyframe_redundancy, T, cand, lists, own)
    assert int(seq["erased"].sum()) >= 2 and int(seq["bad"].sum()) - int(T.bad.sum()) >= 1
    for k in ("verdict", "erased", "n_counted", "n_redundant"):
        assert np.array_equal(seq[k], msk[k]), k
    removed = np.zeros(T.n_keyframes, bool)
    removed[cand[seq["erased"] != 0]] = True
    lost_low = np.array([removed[o].any() and int(np.where(s[~removed[o]] != 0, 2, 1).sum()) <= 2 for o, s in zip(m["observers"], m["stereo"])])
    assert np.array_equal(lost_low | (T.bad != 0), seq["bad"] != 0)
    one = S.ref_keyframe_redundancy(T, cand, lists, own)
    assert not np.array_equal(one["cull"], seq["verdict"])                 # a single unmasked call decides differently


def test_sequential_erasure_keeps_a_not_erase_keyframe_unmasked():
    m = S.culling_map(S.CULLING_SEEDS[0])
    cand, lists, own = S.candidates(m)
    free = S.ref_sequential_culling(m["table"], cand, lists, own)
    first = int(np.nonzero(free["erased"])[0][0])
    ne = np.zeros(len(cand), np.uint8)
    ne[first] = 1
    seq = S.ref_sequential_culling(m["table"], cand, lists, own, not_erase=ne)
    msk = S.masked_culling(S.ref_keyframe_redundancy, m["table"], cand, lists, own, not_erase=ne)
    assert seq["verdict"][first] == 1 and seq["erased"][first] == 0
    for k in ("verdict", "erased", "n_counted", "n_redundant"):
        assert np.array_equal(seq[k], msk[k]), k
    assert not np.array_equal(seq["erased"], free["erased"])


def test_the_observers_order_changes_the_normals_bits():
    """The float sum over the observers is ordered: reversing every point's span changes the normal of at least one of 200 points, which
    is why the ABI takes the order of the reference's container and does not sort."""
    from ydorbslam_amd.map_maintenance import ObservationTable
    m = S.random_map(8, 30, 200, 3, 12)
    a = S.ref_update_normal_depth(m["table"], m["pos"], m["centre"], m["ref_kf"], m["ref_level"], S.scale_factors())
    rev = ObservationTable(30, [o[::-1] for o in m["observers"]], [l[::-1] for l in m["levels"]], [s[::-1] for s in m["stereo"]])
    b = S.ref_update_normal_depth(rev, m["pos"], m["centre"], m["ref_kf"], m["ref_level"], S.scale_factors())
    differs = (a["normal"].view(np.uint32) != b["normal"].view(np.uint32)).any(axis=1)
    assert differs.any()
    assert np.array_equal(a["max_distance"].view(np.uint32), b["max_distance"].view(np.uint32))      # the distances do not depend on it
    assert np.allclose(a["normal"], b["normal"], rtol=0, atol=1e-6)


def _raises(match, fn, *a, **k):
    import ydorbslam_amd as y
    with pytest.raises(y.YdorbError, match=match) as e:
        fn(*a, **k)
    assert "ydorb error -1:" in str(e.value)                               # YDORB_ERR_INVALID_ARG, not the missing device


def test_every_validation_error_comes_before_a_device_is_required():
    import ydorbslam_amd as y
    from ydorbslam_amd import map_maintenance as M
    m = S.random_map(2, 6, 20, 1, 4)
    T, sf = m["table"], S.scale_factors()
    nd = (m["pos"], m["centre"], m["ref_kf"], m["ref_level"], sf)
    _raises("device 16 outside", M.update_normal_depth, T, *nd, device=16)
    _raises("device -1 outside", M.update_normal_depth, T, *nd, device=-1)
    _raises("n_levels 9 outside", M.update_normal_depth, T, *nd[:4], np.ones(9, f32))
    lv = np.minimum(m["ref_level"], 2)
    lv[5] = 3
    _raises("point 5: reference level 3 >= n_levels 3", M.update_normal_depth, T, m["pos"], m["centre"], m["ref_kf"], lv, sf[:3])
    rk = m["ref_kf"].copy(); rk[7] = 6
    _raises("point 7: reference keyframe slot 6", M.update_normal_depth, T, m["pos"], m["centre"], rk, m["ref_level"], sf)
    broken = M.ObservationTable.from_arrays(6, T.obs_start.copy(), T.obs_kf.copy(), T.obs_level, T.bad)
    broken.obs_kf[3] = 6
    _raises("observation 3: keyframe slot 6", M.update_normal_depth, broken, *nd)
    broken = M.ObservationTable.from_arrays(6, T.obs_start.copy(), T.obs_kf, T.obs_level, T.bad)
    broken.obs_start[0] = 1
    _raises(r"obs_start\[0\] is 1", M.covisibility, broken, [0], [[0]])
    broken.obs_start[0], broken.obs_start[4] = 0, broken.obs_start[3] - 1
    _raises("obs_start decreases at 4", M.keyframe_redundancy, broken, [0], [[0]], [[0]])
    _raises(r"query_kf\[1\]: keyframe slot 6", M.covisibility, T, [0, 6], [[0], [1]])
    _raises("list entry 1: point index 20", M.covisibility, T, [0], [[0, 20]], capacities=[5])
    _raises(r"cand_kf\[0\]: keyframe slot -1", M.keyframe_redundancy, T, [-1], [[0]], [[0]])
    _raises("list entry 0: point index -1", M.keyframe_redundancy, T, [1], [[-1]], [[0]])
    _raises("device 16 outside", M.covisibility, T, [0], [[0]], device=16)
    _raises("device 16 outside", M.keyframe_redundancy, T, [0], [[0]], [[0]], device=16)
    null = M.ObservationTable.from_arrays(6, T.obs_start, T.obs_kf, T.obs_level, T.bad)
    null.struct.obs_kf = None
    _raises("null obs_kf", M.covisibility, null, [0], [[0]])
    import ctypes as C
    st = np.zeros(1, np.uint8)
    rc = y.lib().ydorb_map_covisibility(C.byref(T.struct), None, 1, None, None, None, 0, None, None, None, S._p(st))
    assert rc == -1 and b"null query_kf" in y.lib().ydorb_last_error()
    rc = y.lib().ydorb_map_release(16)
    assert rc == -1


def test_capacity_bound_is_tight_and_python_and_header_agree_on_the_window():
    from ydorbslam_amd import map_maintenance as M
    T = _table(4, [[0, 1, 2], [], [3, 1]])
    assert M.capacity_bounds(T, [[0, 2], [1], [0, 0, 0]]) == [3, 0, 3]
    hdr = open(os.path.join(ROOT, "ydorbslam_amd", "csrc", "map_table.h")).read()
    import re
    assert int(re.search(r"constexpr int kCovisWindow = (\d+);", hdr).group(1)) == M.COVIS_WINDOW


def test_map_maintenance_adapters_typecheck():
    """include/ydorb/mapPoint.hpp, keyFrame.hpp and keyFrameCullingImpl against declarations of the KeyFrame / MapPoint members they use."""
    H = os.path.join(ROOT, "tests", "cpu_harness")
    subprocess.check_call(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-I" + os.path.join(H, "mock"), os.path.join(H, "mapmaint_syntax_check.cpp")])


def test_table_checks_in_a_sanitized_program(tmp_path):
    """Validation cases, the capacity bound and offsets at and past INT32_MAX formed without allocating, over map_table.h alone.  The
    program is its own process; nothing is loaded into this one."""
    exe = str(tmp_path / "map_table_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", CHECK_SRC, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.splitlines()
    assert lines[-1] == "0 failed" and len(lines) == 33
