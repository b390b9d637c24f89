"""The resident forms of the two fuse adapters EXECUTED on the GPU through the C++ adapters (tests/cpp_host/localmapping_resident_run.cpp):
fuseByProjection(Mirror&, ...) / fuseBySim3(Mirror&, ...) of include/ydorb/orbMatcher.hpp and both directions of
searchInNeighborsImpl(Mirror&, ...) of include/ydorb/localMapping.hpp over a MapMirror with attributes, features and descriptors leave
the objects - observations, keyframe map-point vectors, replaced-by links - and the return values exactly as the flat adapters, called
once per target, leave a second copy of the same scene; and every verify*() of the mirror is empty afterwards: the touches the
overloads make are complete."""
import os
import subprocess

import pytest

from frustum_support import ROOT

pytestmark = pytest.mark.gpu
SRC = os.path.join(ROOT, "tests", "cpp_host", "localmapping_resident_run.cpp")


@pytest.fixture(scope="module")
def figures(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fuseres") / "localmapping_resident_run")
    lib_dir = os.path.join(ROOT, "ydorbslam_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpu_harness", "mockrt"),
                           "-I" + os.path.join(ROOT, "include"), SRC, "-o", out, "-L" + lib_dir, "-l:libydorb.so", "-Wl,-rpath," + lib_dir])
    r = subprocess.run([out], stdout=subprocess.PIPE, text=True, check=True, timeout=120)
    print(r.stdout)
    return {w[0]: int(w[1]) for w in (ln.split() for ln in r.stdout.splitlines())}


def test_search_in_neighbors_over_the_mirror_equals_the_flat_calls(figures):
    f = figures
    assert f["worlds_equal_before"] == 1 and f["points"] > 150 and f["verify_before"] == 0
    assert f["direction1_counts_same"] == 1 and f["direction1_fused"] >= 10
    assert f["direction2_resident"] == f["direction2_flat"] >= 10
    assert f["state_same"] == 1 and f["replaced"] >= 5                           # some points replaced another, some gained an observation


def test_the_overloads_touch_everything_they_change(figures):
    f = figures
    assert f["verify_after"] == 0 and f["sim3_verify_after"] == 0
    assert f["features_resident"] > 300 and f["last_feat_sync_bytes"] == 0       # the features went up once, before the searches


def test_fuse_by_sim3_over_the_mirror_equals_the_flat_calls(figures):
    f = figures
    assert f["sim3_counts_same"] == 1 and f["sim3_fused"] >= 10 and f["sim3_state_same"] == 1
