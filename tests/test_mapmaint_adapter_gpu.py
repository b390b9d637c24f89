"""The map-maintenance adapters (include/ydorb/mapPoint.hpp, keyFrame.hpp, keyFrameCullingImpl of localMapping.hpp) EXECUTED on the GPU
(tests/cpp_host/mapmaint_run.cpp on stand-ins of KeyFrame / MapPoint that carry data).  The stand-ins' observation containers are
std::maps keyed by pointer; the program dumps their iteration order and the Python replay follows it.  updateNormalAndDepthBatch applies
the bits of the ctypes path, covisibilityCounter returns the same map, and keyFrameCullingImpl flags the keyframes of the
sequential-erasure routine (tests/mapmaint_ref) in the same order."""
import numpy as np
import pytest

import mapmaint_support as S

pytestmark = pytest.mark.gpu
SF = S.scale_factors()
CURRENT = 0
COVISIBLE = [7, 3, 0, 12, 25, 1, 9, 30, 18, 2, 39, 21, 5, 14, 33, 8, 27, 11, 36, 4]     # the first keyframe of the map is among them: skipped
QUERIES = [0, 5, 17, 39]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return S.build_adapter_exe(str(tmp_path_factory.mktemp("mm") / "mapmaint_run"))


def _scene(not_erase=()):
    m = S.random_map(3, 40, 600, 0, 12, 0.5, bad_share=0.03, level_spread=1)     # some points without observations, some bad
    return S.adapter_scene(m, 8.0, seed=1, not_erase=not_erase)


@pytest.fixture(scope="module")
def free_run(exe, tmp_path_factory):
    scene = _scene()
    return scene, S.run_adapters(exe, str(tmp_path_factory.mktemp("run")), scene, CURRENT, COVISIBLE, QUERIES, SF)


def _culling_reference(scene, order, not_erase=None):
    T, _ = S.scene_table(scene, order)
    cand = np.array([k for k in COVISIBLE if k != 0], np.int32)
    lists, own = S.scene_lists(scene, cand, True)
    ne = None if not_erase is None else np.array([1 if k in not_erase else 0 for k in cand], np.uint8)
    return T, cand, lists, own, S.ref_sequential_culling(T, cand, lists, own, 3, ne)


def test_normal_and_depth_batch_applies_the_bits_of_the_ctypes_path(free_run):
    from ydorbslam_amd import map_maintenance as M
    scene, got = free_run
    T, ref_level = S.scene_table(scene, got["order"])
    pos = np.array([p["pos"] for p in scene["points"]], np.float32)
    centre = np.array([k["centre"] for k in scene["kfs"]], np.float32)
    want = M.update_normal_depth(T, pos, centre, [p["ref_kf"] for p in scene["points"]], ref_level, SF)
    assert np.array_equal(got["applied"] != 0, want["status"] == 0) and {0, 1, 2} == set(want["status"].tolist())
    S.same_normal_depth(dict(got, status=want["status"]), want)           # unapplied points were dumped as zeros, which the entry returns too
    S.same_normal_depth(want, S.ref_update_normal_depth(T, pos, centre, [p["ref_kf"] for p in scene["points"]], ref_level, SF))
    assert any(list(o) != sorted(o) for o in got["order"])                # the containers do not iterate by id


def test_covisibility_counter_returns_the_map_of_the_ctypes_path(free_run):
    from ydorbslam_amd import map_maintenance as M
    scene, got = free_run
    T, _ = S.scene_table(scene, got["order"])
    lists, _ = S.scene_lists(scene, QUERIES, False)
    want = M.covisibility(T, QUERIES, lists)
    for q, w in enumerate(want):
        assert w["status"] == 0 and got["counters"][q] == dict(zip(w["kf"].tolist(), w["weight"].tolist())), q
        assert len(w["kf"]) > 20 and QUERIES[q] not in got["counters"][q]


def test_culling_flags_the_keyframes_of_sequential_erasure_in_order(free_run):
    from ydorbslam_amd import map_maintenance as M
    scene, got = free_run
    T, cand, lists, own, seq = _culling_reference(scene, got["order"])
    assert got["flagged"] == cand[seq["verdict"] != 0].tolist() and len(got["flagged"]) >= 2
    bad = np.zeros(len(scene["kfs"]), np.int32)
    bad[cand[seq["erased"] != 0]] = 1
    assert np.array_equal(got["bad"], bad) and 0 not in got["flagged"]
    first = M.keyframe_redundancy(T, cand, lists, own)                    # the unmasked first call alone decides differently
    assert not np.array_equal(first["cull"], seq["verdict"])
    later = np.nonzero(first["cull"] != seq["verdict"])[0]
    assert later[0] > np.nonzero(seq["erased"])[0][0]                    # ... for a candidate after the first one that was erased


def test_a_not_erase_keyframe_is_flagged_but_stays_unmasked(exe, free_run, tmp_path):
    _, free = free_run
    protected = free["flagged"][0]
    scene = _scene(not_erase=(protected,))
    got = S.run_adapters(exe, str(tmp_path), scene, CURRENT, COVISIBLE, QUERIES, SF)
    _, cand, _, _, seq = _culling_reference(scene, got["order"], not_erase=(protected,))
    assert got["flagged"] == cand[seq["verdict"] != 0].tolist()
    assert got["flagged"][0] == protected and got["bad"][protected] == 0
    bad = np.zeros(len(scene["kfs"]), np.int32)
    bad[cand[seq["erased"] != 0]] = 1
    assert np.array_equal(got["bad"], bad)
    assert got["flagged"] != free["flagged"]                              # its observations stayed, so later verdicts differ
