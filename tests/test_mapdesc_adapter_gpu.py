"""ydorb::adapter::MapMirror with descriptors enabled (include/ydorb/mapMirror.hpp) EXECUTED on the GPU on stand-ins of KeyFrame /
MapPoint (tests/cpp_host/mapdesc_run.cpp): after everything was touched, after a keyframe insertion, after a fuse that replaces points
and after a keyframe cull, the descriptor every touched point receives equals what the stand-in's own sequential
computeDistinctiveDescriptors leaves in m_descriptor, and verifyDescriptors() is clean.  The program compares exactly."""
import os
import subprocess

import pytest

from mapmaint_support import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mapdesc") / "mapdesc_run")
    lib_dir = os.path.join(ROOT, "ydorbslam_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpu_harness", "mockrt"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp_host", "mapdesc_run.cpp"), "-o", exe,
                           "-L" + lib_dir, "-l:libydorb.so", "-Wl,-rpath," + lib_dir])
    r = subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True)
    return {ln.split()[0]: int(ln.split()[1]) for ln in r.stdout.splitlines()}


@pytest.mark.parametrize("phase", ["A", "B", "C", "D", "E"])
def test_the_mirror_gives_every_touched_point_the_sequential_descriptor(run, phase):
    """A: everything touched; B: a keyframe inserted; C: points replaced by a fuse, one forgotten; D: a keyframe erased and one flagged
    bad, the points they showed; E: every point once more."""
    assert run[phase + "_same"] == 1 and run[phase + "_views_agree"] == 1 and run[phase + "_verify_differences"] == 0
    assert run[phase + "_applied"] == run[phase + "_updated"] > 0


def test_the_steps_happened(run):
    assert run["A_updated"] > 200 and run["B_touched"] >= 8 and run["C_replaced"] == 20 and run["D_touched"] >= 10
    assert run["E_updated"] < run["A_updated"] + 5                            # replaced points went bad
    assert run["stats_views"] > 800 and run["stats_descriptors"] == 29 * 64 and run["stats_repacks"] >= 2


def test_a_missed_touch_is_named_by_verify_descriptors(run):
    assert run["verify_named"] == 1 and run["verify_named_slot"] == run["missed_touch_slot"] >= 0 and run["verify_after_the_touch"] == 0
