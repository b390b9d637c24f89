"""The resident form of Tracking::searchLocalPoints EXECUTED on the GPU through the C++ adapters (tests/cpp_host/tracking_resident_run.cpp):
updateLocalPointsImpl and searchLocalPointsImpl(Mirror&, ...) of include/ydorb/tracking.hpp over a MapMirror with enableAttributes()
(include/ydorb/mapMirror.hpp) give the frame's map-point vector, the track members, the visibility counters and the last-seen frame ids
that the flat searchLocalPointsImpl gives on a second copy of the same scene, with no map value uploaded by the search.  The scene is
the one of test_tracking_adapter_gpu.py, whose scenario builder is used as it is."""
import os
import subprocess

import pytest

import test_tracking_adapter_gpu as T
from frustum_support import ROOT

pytestmark = pytest.mark.gpu
SRC = os.path.join(ROOT, "tests", "cpp_host", "tracking_resident_run.cpp")


@pytest.fixture(scope="module")
def figures(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("trkres")
    out, inp = str(tmp / "tracking_resident_run"), str(tmp / "in.bin")
    lib_dir = os.path.join(ROOT, "ydorbslam_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpu_harness", "mockrt"),
                           "-I" + os.path.join(ROOT, "include"), SRC, "-o", out, "-L" + lib_dir, "-l:libydorb.so", "-Wl,-rpath," + lib_dir])
    sc = T._scenario()
    open(inp, "wb").write(T._blob(sc))
    r = subprocess.run([out, inp], stdout=subprocess.PIPE, text=True, check=True, timeout=120)
    print(r.stdout)
    return sc, {w[0]: int(w[1]) for w in (ln.split() for ln in r.stdout.splitlines())}


def test_the_resident_overload_equals_the_flat_one(figures):
    _, f = figures
    assert f["matches_resident"] == f["matches_flat"] >= 50
    assert f["frame_map_points_same"] == 1 and f["track_members_same"] == 1 and f["visible_and_last_seen_same"] == 1
    assert f["in_view"] > 100


def test_the_local_points_come_from_the_rows_and_nothing_of_the_map_goes_up(figures):
    sc, f = figures
    n_bad = int((sc["pts"]["bad"][:sc["n_loc"]] != 0).sum())
    assert n_bad > 0 and f["local_points"] == sc["n_loc"] - n_bad and f["local_points_in_order"] == 1 and f["seen"] == 1
    assert f["last_attr_sync_bytes"] == 0 and f["last_sync_bytes"] == 0          # the search's sync found nothing staged
    assert f["attr_growths"] >= 1 and f["attr_capacity_is_point_capacity"] == 1  # the arena followed the point table while the scene was loaded


def test_verify_attributes_names_a_change_without_its_touch(figures):
    _, f = figures
    assert f["verify_differences"] == 0 and f["verify_attributes_differences"] == 0
    assert f["verify_attributes_named"] == 1 and f["verify_attributes_after_the_touch"] == 0


def test_a_forgotten_slot_taken_again_reads_as_no_attributes_until_they_are_set(figures):
    """forget(), then the slot reused before the next flush by a point whose descriptor is an empty matrix: flags 0 and status 7 before a
    touch, the geometry alone (flag 1, still status 7 in the fused search) after touchAttributes, complete and in view once the
    descriptor is set and touched."""
    _, f = figures
    assert f["slot_reused"] == 1
    assert f["reused_slot_flags_before_a_touch"] == 0 and f["reused_slot_status_before_a_touch"] == 7
    assert f["reused_slot_flags_with_an_empty_descriptor"] == 1 and f["reused_slot_status_with_an_empty_descriptor"] == 7
    assert f["verify_attributes_names_the_missing_group"] == 1
    assert f["reused_slot_flags_after_the_descriptor"] == 3 and f["reused_slot_status_after_the_descriptor"] == 0
    assert f["verify_attributes_at_the_end"] == 0
