"""The resident overload createNewMapPointsImpl(Mirror&, ...) of include/ydorb/localMapping.hpp EXECUTED on the GPU
(tests/cpp_host/createpoints_resident_run.cpp, on stand-ins of KeyFrame / MapPoint / Map that carry data) beside the flat
createNewMapPointsImpl on a second copy of the same keyframes: identical created points - positions bit for bit, both observations,
the order - identical keyframe map-point vectors, the abort check, and a mirror that verifies clean afterwards."""
import os
import subprocess

import pytest

import mapdb_tri_support as T
from triangulate_support import ROOT

pytestmark = pytest.mark.gpu
SRC = os.path.join(ROOT, "tests", "cpp_host", "createpoints_resident_run.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cnp") / "createpoints_resident_run")
    lib_dir = os.path.join(ROOT, "ydorbslam_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpu_harness", "mockrt"),
                           "-I" + os.path.join(ROOT, "include"), SRC, "-o", out, "-L" + lib_dir, "-l:libydorb.so", "-Wl,-rpath," + lib_dir])
    return out


@pytest.fixture(scope="module")
def scene():
    return T.Scene(seed=15, n=200, n_nb=4, mapped=0.0)


def _run(exe, tmp, scene, abort_after):
    inp = os.path.join(tmp, "in.bin")
    open(inp, "wb").write(T.scenario_blob(scene, abort_after))
    out = subprocess.run([exe, inp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, out.stderr
    return {ln.split()[0]: int(ln.split()[1]) for ln in out.stdout.splitlines()}


def test_the_resident_overload_creates_the_flat_body_s_points(exe, scene, tmp_path, oracle_lib):
    want = scene.reference(oracle_lib)
    r = _run(exe, str(tmp_path), scene, -1)
    assert r["state_same"] == 1 and r["created_flat"] == r["created_resident"] == r["map_points"] == r["recent"] == int(want["n_accepted"].sum())
    assert [r["created_with_%d" % k] for k in range(1, 5)] == want["n_accepted"].tolist() and min(want["n_accepted"]) >= 5
    assert r["abort_calls_flat"] == r["abort_calls_resident"] == 3
    assert r["verify_after"] == 0 and r["bow_entries_resident"] == sum(len(k["bow"]) for k in scene.kfs)
    assert r["second_call_same"] == 1


def test_abort_check_turning_true_after_the_second_neighbour(exe, scene, tmp_path, oracle_lib):
    want = scene.reference(oracle_lib)
    r = _run(exe, str(tmp_path), scene, 2)
    assert r["state_same"] == 1 and r["created_flat"] == r["created_resident"] == int(want["n_accepted"][:2].sum())
    assert r["abort_calls_flat"] == r["abort_calls_resident"] == 2 and r["created_with_3"] == r["created_with_4"] == 0
    assert r["verify_after"] == 0
    assert r["second_call_same"] == 1 and r["second_call_created"] >= 5          # the rest, on rows whose entries were staged one by one
