"""The resident overloads searchByBowInTwoKeyFrames(Mirror&, ...) / searchByBowInKeyFrameAndFrame(Mirror&, ...) of
include/ydorb/orbMatcher.hpp and trackReferenceKeyFrameSearchImpl of include/ydorb/tracking.hpp EXECUTED on the GPU
(tests/cpp_host/bowsearch_resident_run.cpp, on stand-ins of KeyFrame / MapPoint / Frame that carry data) beside the flat adapters called
once per candidate on a second copy of the same keyframes: 5 candidates, a tenth of the points bad, one bad candidate keyframe.  The
match vectors hold the same points' ids, the counts are equal, the mirror verifies clean afterwards, and a mirror without enableBow()
refuses."""
import os
import subprocess

import numpy as np
import pytest

import mapdb_bowsearch_support as B
from triangulate_support import ROOT

pytestmark = pytest.mark.gpu
SRC = os.path.join(ROOT, "tests", "cpp_host", "bowsearch_resident_run.cpp")
BAD_CANDIDATE = 3


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bows") / "bowsearch_resident_run")
    lib_dir = os.path.join(ROOT, "ydorbslam_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpu_harness", "mockrt"),
                           "-I" + os.path.join(ROOT, "include"), SRC, "-o", out, "-L" + lib_dir, "-l:libydorb.so", "-Wl,-rpath," + lib_dir])
    return out


def _features(side):
    ids, start, feat = B.csr(side["bow"])
    b = [np.array([len(side["kps"])], np.int32).tobytes(), side["kps"].tobytes(), side["desc"].tobytes(), np.array([len(ids)], np.int32).tobytes()]
    for i, node in enumerate(ids):
        f = feat[start[i]:start[i + 1]].astype(np.uint32)
        b += [np.array([node], np.uint32).tobytes(), np.array([len(f)], np.int32).tobytes(), f.tobytes()]
    return b


def scenario_blob(scene):
    """Points (the bad flags; a mirror has no slot that was never set, so those read as bad points), keyframes with their rows, the frame."""
    b = [np.array([scene.n_points], np.int32).tobytes(), scene.bad.tobytes(), np.array([len(scene.kfs)], np.int32).tobytes()]
    for k, kf in enumerate(scene.kfs):
        b += [np.array([1 if k == BAD_CANDIDATE else 0], np.int32).tobytes()] + _features(kf) + [kf["row"].astype(np.int32).tobytes()]
    return b"".join(b + _features(scene.frame))


def test_the_resident_overloads_fill_the_flat_adapters_match_vectors(exe, tmp_path):
    scene = B.Scene(seed=41, n=200, n_cand=5)
    inp = os.path.join(str(tmp_path), "in.bin")
    open(inp, "wb").write(scenario_blob(scene))
    out = subprocess.run([exe, inp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, out.stderr
    r = {ln.split()[0]: int(ln.split()[1]) for ln in out.stdout.splitlines()}
    assert r["candidates"] == 5 and r["bad_candidates"] == r["bad_candidates_unusable"] == 1
    assert r["loop_same"] == 1 and r["reloc_same"] == 1 and r["reference_same"] == 1
    assert r["loop_min"] >= 10 and r["reloc_min"] >= 10 and r["reference_matches"] >= 10     # the comparison is not between empty vectors
    assert r["verify_after"] == 0
    assert r["bad_point_followed"] == 1
    assert r["refused_without_bow"] == 2
    assert r["bad_first_answers"] == 1
