"""The C++ adapters of Tracking::updateLocalMap EXECUTED on the GPU: updateLocalKeyFramesImpl / updateLocalPointsImpl
(include/ydorb/tracking.hpp) over MapMirror's keyframe rows (include/ydorb/mapMirror.hpp) beside the two reference loops written out
on the same stand-ins (tests/cpp_host/localmap_run.cpp), in four states.  Every comparison is exact."""
import os
import subprocess

import pytest

from mapmaint_support import ROOT

pytestmark = pytest.mark.gpu
SRC = os.path.join(ROOT, "tests", "cpp_host", "localmap_run.cpp")


@pytest.fixture(scope="module")
def figures(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("localmap") / "localmap_run")
    lib_dir = os.path.join(ROOT, "ydorbslam_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpu_harness", "mockrt"),
                           "-I" + os.path.join(ROOT, "include"), SRC, "-o", out, "-L" + lib_dir, "-l:libydorb.so", "-Wl,-rpath," + lib_dir])
    r = subprocess.run([out], stdout=subprocess.PIPE, text=True, check=True, timeout=120)
    print(r.stdout)
    return {w[0]: int(w[1]) for w in (ln.split() for ln in r.stdout.splitlines())}


@pytest.mark.parametrize("state", "ABCD")
def test_local_map_equals_the_reference_loops(figures, state):
    """A: everything touched; B: addMapPoint / erase / replace, a new keyframe and bad points with their touches; C: a keyframe forgotten
    and its slot reused; D: after the missed touch was made up for."""
    for what in ("local_keyframes_same", "reference_keyframe_same", "local_points_same", "seen_same", "nulled_same"):
        assert figures["%s_%s" % (state, what)] == 1, what
    assert figures[state + "_verify_rows_differences"] == 0 and figures[state + "_verify_differences"] == 0
    # the scene exercises what it is meant to: frames past the 80-keyframe stop, nulled bad entries, seen points, a real local map
    assert figures[state + "_frames_past_80"] >= 2 and figures[state + "_nulled"] > 0 and figures[state + "_seen"] > 100
    assert figures[state + "_local_keyframes"] > 150 and figures[state + "_local_points"] > 3000


def test_the_mutations_ran_and_a_slot_was_reused(figures):
    assert min(figures["mutations_added"], figures["mutations_erased"], figures["mutations_replaced"]) >= 20 and figures["slot_reused"] == 1
    assert figures["row_stats_header_growths"] >= 1 and figures["row_stats_repacks"] >= 1


def test_a_mutation_without_its_touch_is_named_by_verify_rows(figures):
    assert figures["verify_rows_named"] == 1 and figures["verify_rows_named_slot"] == figures["missed_touch_slot"] >= 0
    assert figures["verify_rows_after_the_touch"] == 0
