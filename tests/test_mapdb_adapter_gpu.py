"""ydorb::adapter::MapMirror (include/ydorb/mapMirror.hpp) EXECUTED on the GPU beside the three flattening adapters, on the same
stand-ins of KeyFrame / MapPoint in one program (tests/cpp_host/mapdb_run.cpp).  The program compares exactly (applied flags, float bit
patterns, counter maps, the flagged keyframes in order) after everything was touched, after a round of mutations with their touches and
after a slot was reused, and then makes one mutation without its touch."""
import pytest

import mapdb_support as D
import mapmaint_support as S
from test_mapmaint_adapter_gpu import COVISIBLE, CURRENT, QUERIES, SF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("mirror"))
    exe = D.build_mirror_exe(tmp + "/mapdb_run")
    m = S.random_map(3, 40, 600, 0, 12, 0.5, bad_share=0.03, level_spread=1)     # test_mapmaint_adapter_gpu's scene
    return D.run_mirror(exe, tmp, S.adapter_scene(m, 8.0, seed=1), CURRENT, COVISIBLE, QUERIES, SF)


@pytest.mark.parametrize("phase", ["A", "B", "C"])
def test_the_three_mirror_calls_equal_the_three_adapters(run, phase):
    """A: everything touched; B: after observations added and erased, a point set bad, positions written back, a pose moved and a
    keyframe erased, each with its touch; C: after a forgotten point's slot was taken by a new point."""
    assert run[phase + "_normal_same"] == 1 and run[phase + "_covisibility_same"] == 1 and run[phase + "_culling_same"] == 1
    assert run[phase + "_normal_updated"] > 500 and run[phase + "_covisibility_connections"] > 60 and run[phase + "_culling_flagged"] >= 2
    assert run[phase + "_verify_differences"] == 0


def test_the_mutations_happened_and_the_small_handle_grew(run):
    assert run["mutations_added"] == 40 and run["mutations_erased"] == 40 and run["erased_keyframe"] in COVISIBLE and run["slot_reused"] == 1
    assert run["B_normal_updated"] != run["A_normal_updated"]                  # points went bad, a keyframe's observations left
    assert run["stats_point_table_growths"] >= 1 and run["stats_keyframe_table_growths"] >= 1 and run["stats_repacks"] >= 1


def test_a_missed_touch_is_named_by_verify_and_fails_nothing(run):
    assert run["verify_named"] == 1 and run["verify_named_slot"] == run["missed_touch_slot"] >= 0
    assert run["missed_touch_points_that_differ"] == 1 and run["missed_touch_differs_at_victim"] == 1
    assert run["verify_after_the_touch"] == 0
