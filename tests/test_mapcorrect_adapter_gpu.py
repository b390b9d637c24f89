"""The three map-correction methods of ydorb::adapter::MapMirror (include/ydorb/mapMirror.hpp) EXECUTED on the GPU beside the
reference's loops A, B, C written plainly on the same stand-ins of KeyFrame / MapPoint in one program (tests/cpp_host/mapcorrect_run.cpp),
the per-point updateNormalAndDepth of the loops through the flattening adapter.  The program compares the objects' whole state exactly
(positions, normals, distances, marks, poses, centres) and asks verify() after every step."""
import pytest

import mapcorrect_support as K
import mapmaint_support as S

pytestmark = pytest.mark.gpu
CURRENT = 17                                                      # not keyframe 0: a fresh point's correction mark is 0
COVISIBLE = [7, 3, 22, 12, 25, 1, 9, 30, 18, 2, 39, 21, 5, 14, 33, 8, 27, 11, 36, 4]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("mapcorrect"))
    exe = K.build_run_exe(tmp + "/mapcorrect_run")
    m = S.random_map(3, 40, 600, 0, 12, 0.5, bad_share=0.03, level_spread=1)
    return K.run_adapter(exe, tmp, S.adapter_scene(m, 8.0, seed=1), CURRENT, COVISIBLE)


def test_the_loaded_mirror_is_in_step(run):
    assert run["loaded_verify_differences"] == 0 and run["stats_point_table_growths"] >= 1


@pytest.mark.parametrize("loop, least", [("A", 150), ("B", 500), ("C", 300)])
def test_each_adapter_method_leaves_the_state_the_reference_loop_leaves(run, loop, least):
    assert run[loop + "_same"] == 1
    assert run[loop + "_corrected"] >= least and run[loop + "_points_moved"] >= run[loop + "_corrected"] - 5
    assert run[loop + "_verify_differences"] == 0                  # right after the method, with no touchPosition
    assert run[loop + "_verify_after_reference"] == 0              # and the reference loop's objects are what the table holds


def test_loop_c_skipped_the_keyframes_that_were_not_reached(run):
    assert run["C_not_reached"] == 8 and run["C_corrected"] < 520
