"""The resident table's keyframe rows without a GPU: the sanitized stand-alone check of ydorbslam_amd/csrc/mapdb_rows_host.h
(validation, coalescing, delta packing, pool policy, the seeded sequence against a naive model) and of the CPU restatement of the two
local-map queries (tests/cpu_harness/mapdb_rows_check.cpp), and what the new C entries do on a machine with no device.  The program is
its own process: nothing is loaded into this one under a sanitizer."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mapdb_rows_support as R
from mapmaint_support import ROOT


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mapdbrows") / "mapdb_rows_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", R.CHECK_SRC, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    return r.stdout.splitlines()


def _case(report, name):
    hits = [ln for ln in report if ln.startswith(name)]
    assert len(hits) == 1 and " ok" in hits[0] and "FAILED" not in hits[0], (name, hits)
    return hits[0]


def test_rows_check_runs_clean_under_the_sanitizers(report):
    cases = [ln for ln in report if not ln.startswith("trace ")]
    assert cases[-1] == "0 failed" and len(cases) == 50 and not any("FAILED" in ln or "MISMATCH" in ln for ln in report)


def test_every_validation_message(report):
    for name, text in (("row_start[0] != 0", "row_start[0] is 1, not 0"), ("row_start decreases", "row_start decreases at 2"),
                       ("negative keyframe slot", "kf_slots[1]: negative keyframe slot -3"),
                       ("point slot past n_points", "point slot 500 outside -1..499; set the point before a row names it"),
                       ("point slot below -1", "point slot -2 outside -1..499"), ("null row_start", "null row_start"),
                       ("null kf_slots", "null kf_slots"), ("null point_slot", "null point_slot"), ("negative n", "negative number of keyframe slots: -1"),
                       ("idx past the row", "index 3 outside the row of 3 entries"), ("idx negative", "index -1 outside the row of 3 entries"),
                       ("idx of a keyframe with no row", "outside the row of 0 entries"), ("idx of a keyframe slot past the table", "outside the row of 0 entries"),
                       ("entry: negative keyframe slot", "negative keyframe slot -1"),
                       ("entry: point slot past n_points", "set the point before a row names it"), ("entry: null arrays", "null kf_slot, idx or point_slot"),
                       ("entry: negative n", "negative number of row entries: -2"),
                       ("a row pool past INT32_MAX entries", "2147483648 entries, past INT32_MAX"),
                       ("query keyframe slot out of range", "keyframe slot 3 outside 0..2"), ("query null kf_slots", "null kf_slots"),
                       ("query negative n_kf", "negative number of keyframe slots"), ("seen slot out of range", "point slot 500 outside -1..499"),
                       ("null seen_points", "null seen_points")):
        assert text in _case(report, name)


def test_coalescing_rejection_and_upload_accounting(report):
    for name in ("coalescing: a row set three times costs the last row only", "coalescing: an entry change after a staged row lands in it",
                 "coalescing: one (keyframe, index) changed twice gives one record", "coalescing: a row staged after an entry change supersedes it",
                 "stats count the staged row", "a refused call stages nothing", "a refused entry call stages nothing", "the rejected calls staged nothing",
                 "... and the rows are what they were", "nothing dirty: last_row_sync_bytes == 0", "a keyframe slot never set has length 0",
                 "a row of length 0 erases", "clear ", "clear, then reuse", "three touched rows: the same bytes at 10 and 1 000 keyframes"):
        _case(report, name)


def test_the_seeded_sequence_equals_the_model_and_meets_every_path(report):
    for name in ("sequence: every sync equals the model", "sequence: a repack that kept the capacity", "sequence: a repack that grew the capacity",
                 "sequence: a keyframe-table growth"):
        _case(report, name)
    trace = R.parse_trace(ln for ln in report if ln.startswith("trace "))
    assert len(trace) == 40 and trace[0]["n_keyframes"] == 40
    last = trace[-1]
    assert min(last["repacks_kept"], last["repacks_grown"], last["header_growths"]) >= 1 and last["n_keyframes"] > 48
    assert min(t["n_entries"] for t in trace) < trace[0]["n_entries"] * 0.5          # most rows were erased once


def test_the_restatement_on_hand_made_cases(report):
    for name in ("restatement: the points of a keyframe set", "restatement: a point twice within one row", "restatement: a keyframe slot with no row",
                 "restatement: the observer counter of a frame"):
        _case(report, name)
    # the same first case through the shared object the GPU tests call
    rows = [np.array(r, np.int32) for r in ([3, -1, 5, 3], [], [5, 6, 2, -1, 0], [4, 4])]
    bad = np.array([0, 0, 1, 0, 0, 0, 0], np.uint8)
    slots, seen = R.ref_points_of_keyframes(rows, bad, [2, 0, 1, 3, 2], [6, -1, 1, 3])
    assert slots.tolist() == [5, 6, 0, 3, 4] and seen.tolist() == [0, 1, 0, 1, 0]


def test_entries_without_a_device_bad_arguments_first_then_no_device():
    import ydorbslam_amd as y
    L = y.lib()
    one, cnt, st = (C.c_int32 * 2)(0, 0), C.c_int32(0), C.c_uint8(0)
    assert L.ydorb_mapdb_set_keyframe_rows(None, None, 0, None, None) == -1 and L.ydorb_mapdb_set_row_entries(None, None, None, None, 0) == -1
    assert L.ydorb_mapdb_export_rows(None, None, None) == -1 and L.ydorb_mapdb_row_stats(None, None) == -1
    assert L.ydorb_mapdb_points_of_keyframes(None, one, -1, None, 0, 0, None, None, C.byref(cnt), C.byref(st)) == -1 and b"negative" in L.ydorb_last_error()
    assert L.ydorb_mapdb_points_of_keyframes(None, one, 1, None, 0, 0, None, None, None, None) == -1 and b"null count or status" in L.ydorb_last_error()
    assert L.ydorb_mapdb_points_of_keyframes(None, None, 1, None, 0, 0, None, None, C.byref(cnt), C.byref(st)) == -1 and b"null kf_slots" in L.ydorb_last_error()
    assert L.ydorb_mapdb_observer_counter(None, -1, one, None, one, None, None, None, None, None) == -1 and b"negative number of lists" in L.ydorb_last_error()
    assert L.ydorb_mapdb_observer_counter(None, 1, None, None, one, None, None, None, None, None) == -1 and b"null list_start" in L.ydorb_last_error()
    rc1 = L.ydorb_mapdb_points_of_keyframes(None, one, 1, None, 0, 0, None, None, C.byref(cnt), C.byref(st))
    rc2 = L.ydorb_mapdb_observer_counter(None, 1, one, None, one, None, None, C.byref(cnt), C.byref(st), None)
    if L.ydorb_device_count() == 0:
        assert rc1 == -2 and rc2 == -2                                         # YDORB_ERR_NO_DEVICE: there is no CPU fallback
    else:
        assert rc1 == -1 and rc2 == -1 and b"null handle" in L.ydorb_last_error()


def test_python_mirror_and_header_agree_on_the_row_stats_layout():
    from ydorbslam_amd._lib import YdMapDbRowStats, YdMapDbStats
    hdr = open(os.path.join(ROOT, "include", "ydorb", "c_api.h")).read()
    body = hdr[hdr.index("typedef struct YdMapDbRowStats {"):hdr.index("} YdMapDbRowStats;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in re.findall(r"int(?:32|64)_t ([^;]+);", body) for n in decl.split(",")]
    assert names == [n for n, _ in YdMapDbRowStats._fields_] and C.sizeof(YdMapDbRowStats) == 56 and C.sizeof(YdMapDbStats) == 72


def test_local_map_adapters_typecheck():
    """The keyframe-row methods of include/ydorb/mapMirror.hpp and updateLocalKeyFramesImpl / updateLocalPointsImpl of
    include/ydorb/tracking.hpp against declarations of the Frame / KeyFrame / MapPoint members they use."""
    H = os.path.join(ROOT, "tests", "cpu_harness")
    subprocess.check_call(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-I" + os.path.join(H, "mock"), os.path.join(H, "localmap_syntax_check.cpp")])
