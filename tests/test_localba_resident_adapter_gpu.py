"""The resident overload of localBundleAdjust EXECUTED on the GPU through the C++ adapters (tests/cpp_host/localba_resident_run.cpp):
localBundleAdjustImpl<Frame>(mirror, ...) of include/ydorb/optimizer.hpp over a MapMirror with descriptors and features leaves the
objects - keyframe poses, point positions, erased observations and map-point vector entries, normals and distances - exactly as the
flat localBundleAdjustImpl leaves a second copy of the same scene, with the stop flag clear and with it set before the solve; every
verify*() of the mirror is empty afterwards, so the touches the overload makes are complete; and MapMirror::localBaGraph refuses a
mirror without enableDescriptors() or without enableFeatures()."""
import os
import subprocess

import pytest

from frustum_support import ROOT

pytestmark = pytest.mark.gpu
SRC = os.path.join(ROOT, "tests", "cpp_host", "localba_resident_run.cpp")


@pytest.fixture(scope="module")
def figures(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lbares") / "localba_resident_run")
    lib_dir = os.path.join(ROOT, "ydorbslam_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpu_harness", "mockrt"),
                           "-I" + os.path.join(ROOT, "include"), SRC, "-o", out, "-L" + lib_dir, "-l:libydorb.so", "-Wl,-rpath," + lib_dir])
    r = subprocess.run([out], stdout=subprocess.PIPE, text=True, check=True, timeout=120)
    print(r.stdout)
    return {w[0]: int(w[1]) for w in (ln.split() for ln in r.stdout.splitlines())}


def test_the_resident_overload_equals_the_flat_one(figures):
    f = figures
    assert f["solved_worlds_equal_before"] == 1 and f["solved_verify_before"] == 0
    assert f["solved_state_same"] == 1
    assert f["solved_values_changed"] > 500 and f["solved_observations_erased"] >= 5     # poses, positions and normals moved; outliers went
    assert f["graph_local"] == 5 and f["graph_fixed"] == 4 and f["graph_points"] > 200 and f["graph_edges"] > 1000


def test_the_overload_touches_everything_it_changes(figures):
    assert figures["solved_verify_after"] == 0 and figures["stopped_verify_after"] == 0


def test_a_stop_set_before_the_solve_changes_nothing_on_either_copy(figures):
    f = figures
    assert f["stopped_worlds_equal_before"] == 1 and f["stopped_verify_before"] == 0
    assert f["stopped_state_same"] == 1 and f["stopped_values_changed"] == 0 and f["stopped_observations_erased"] == 0


def test_the_mirror_refuses_without_descriptors_or_features(figures):
    assert figures["refused_without_descriptors"] == 1 and figures["refused_without_features"] == 1
