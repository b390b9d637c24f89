"""The resident table's descriptor blocks and point views without a GPU: the sanitized stand-alone check of
ydorbslam_amd/csrc/mapdb_desc_host.h (validation, coalescing, delta packing, the pool policy of both relations, the seeded sequence
against a naive model, the host execution of the query against a direct restatement; tests/cpu_harness/mapdb_desc_check.cpp), what the
seven new C entries do on a machine with no device, and the adapter's type check.  The program is its own process: nothing is loaded
into this one under a sanitizer."""
import ctypes as C
import os
import re
import subprocess

import pytest

import mapdb_desc_support as R
from mapmaint_support import ROOT


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mapdbdesc") / "mapdb_desc_check")
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


def test_desc_check_runs_clean_under_the_sanitizers(report):
    cases = [ln for ln in report if not ln.startswith("trace ")]
    assert cases[-1] == "0 failed" and len(cases) == 69 and not any("FAILED" in ln or "MISMATCH" in ln for ln in report)


def test_every_validation_message(report):
    for name, text in (("desc_start[0] != 0", "desc_start[0] is 1, not 0"), ("desc_start decreases", "desc_start decreases at 2"),
                       ("negative keyframe slot", "kf_slots[1]: negative keyframe slot -3"), ("null desc_start", "null desc_start"),
                       ("null kf_slots", "null kf_slots"), ("null desc ", "null desc"), ("blocks: negative n", "negative number of keyframe slots: -1"),
                       ("view_start[0] != 0", "view_start[0] is 2, not 0"), ("view_start decreases", "view_start decreases at 2"),
                       ("negative point slot", "slots[1]: negative point slot -2"),
                       ("point slot past n_points", "point slot 200 outside 0..199; set the point before its views"),
                       ("view_kf past n_keyframes", "view 2: keyframe slot 64 outside 0..63"), ("view_kf negative", "keyframe slot -1 outside 0..63"),
                       ("view_idx negative", "view 1: negative keypoint index -1"),
                       ("a view span longer than 65 535", "a span of 65536 views, more than 65535"), ("null view_start", "null view_start"),
                       ("null slots", "null slots"), ("null view_kf", "null view_kf or view_idx"), ("null view_idx", "null view_kf or view_idx"),
                       ("views: negative n", "negative number of point slots: -2"),
                       ("a view pool past INT32_MAX entries", "2147483648 entries, past INT32_MAX"),
                       ("a descriptor pool past INT32_MAX entries", "2147483648 descriptors, past INT32_MAX"),
                       ("query slot past n_points", "point slot 200 outside 0..199"), ("query slot negative", "point slot -1 outside 0..199"),
                       ("query null slots", "null slots"), ("query null outputs with n > 0", "null output arrays"),
                       ("query negative n", "negative number of point slots: -1"), ("reserve with a pool in use", "the pools are not empty"),
                       ("reserve a negative capacity", "negative capacity"), ("reserve past INT32_MAX", "past INT32_MAX")):
        assert text in _case(report, name)
    for name in ("a view span of 65 535", "a descriptor pool of INT32_MAX entries", "query null outputs with n == 0"):
        _case(report, name)


def test_coalescing_rejection_and_upload_accounting(report):
    for name in ("coalescing: a block set three times costs the last block only", "coalescing: a slot named twice in one call keeps its last views",
                 "stats count what is staged", "a rejected set_point_views stages nothing", "a rejected set_keyframe_descriptors stages nothing",
                 "the rejected calls staged nothing", "... and nothing is dirty", "... and the relations are what they were",
                 "nothing staged: last_desc_sync_bytes == 0", "a slot never set has no views and no block", "delta payload offsets are 16-byte aligned",
                 "a block of length 0 erases the block", "an empty span erases the views", "clear empties both and keeps capacities and counters",
                 "reserve on empty pools", "reserve sets the capacities", "reserve after clear", "clear, then reuse"):
        _case(report, name)


def test_the_host_query_on_hand_made_cases(report):
    for name in ("host query: best is the span position, skipped views counted", "host query: every view skipped is status 2",
                 "host query: idx == len is status 3 with zero rows", "host query: one row wins", "host query: a bad point is status 1",
                 "host query: two rows, the first wins", "host query: a point without views is status 2", "host query: a repeated slot repeats its answer"):
        _case(report, name)


def test_the_seeded_sequence_equals_the_model_and_meets_every_path(report):
    for name in ("sequence: every sync equals the model", "sequence: the host query equals the restatement after every sync",
                 "sequence: the queries met every status", "sequence: a view repack that kept the capacity", "sequence: a view repack that grew the capacity",
                 "sequence: a descriptor repack that kept the capacity", "sequence: a descriptor repack that grew the capacity"):
        _case(report, name)
    trace = R.parse_trace(ln for ln in report if ln.startswith("trace "))
    assert len(trace) == 40 and trace[0]["view_pool_capacity"] > R.SEQUENCE_RESERVE[0] and trace[0]["desc_pool_capacity"] == R.SEQUENCE_RESERVE[1]
    last = trace[-1]
    assert min(last["view_repacks_kept"], last["view_repacks_grown"], last["desc_repacks_kept"], last["desc_repacks_grown"]) >= 1
    assert min(t["n_views"] for t in trace) < trace[0]["n_views"] * 0.5 and min(t["n_descriptors"] for t in trace) < trace[0]["n_descriptors"] * 0.5
    assert trace[-1]["n_descriptors"] > trace[10]["n_descriptors"] * 2          # the culled keyframes came back


def test_entries_without_a_device_bad_arguments_first_then_no_device():
    import ydorbslam_amd as y
    L = y.lib()
    one = (C.c_int32 * 2)(0, 0)
    row, st = (C.c_uint8 * 32)(), C.c_uint8(0)
    assert L.ydorb_mapdb_reserve_descriptors(None, 1, 1) == -1 and b"null handle" in L.ydorb_last_error()
    assert L.ydorb_mapdb_set_keyframe_descriptors(None, None, 0, None, None) == -1 and L.ydorb_mapdb_set_point_views(None, None, 0, None, None, None) == -1
    assert L.ydorb_mapdb_export_views(None, None, None, None) == -1 and L.ydorb_mapdb_export_descriptors(None, None, None) == -1
    assert L.ydorb_mapdb_desc_stats(None, None) == -1 and b"null handle or stats" in L.ydorb_last_error()
    assert L.ydorb_mapdb_distinctive_descriptors(None, one, -1, one, one, row, C.byref(st)) == -1 and b"negative number of point slots" in L.ydorb_last_error()
    assert L.ydorb_mapdb_distinctive_descriptors(None, None, 1, one, one, row, C.byref(st)) == -1 and b"null slots" in L.ydorb_last_error()
    assert L.ydorb_mapdb_distinctive_descriptors(None, one, 1, one, None, row, C.byref(st)) == -1 and b"null output arrays" in L.ydorb_last_error()
    rc = L.ydorb_mapdb_distinctive_descriptors(None, one, 1, one, one, row, C.byref(st))
    if L.ydorb_device_count() == 0:
        assert rc == -2                                                        # YDORB_ERR_NO_DEVICE: there is no CPU fallback
    else:
        assert rc == -1 and b"null handle" in L.ydorb_last_error()


def test_python_mirror_and_header_agree_on_the_desc_stats_layout():
    from ydorbslam_amd._lib import YdMapDbDescStats, YdMapDbRowStats, YdMapDbStats
    hdr = open(os.path.join(ROOT, "include", "ydorb", "c_api.h")).read()
    body = hdr[hdr.index("typedef struct YdMapDbDescStats {"):hdr.index("} YdMapDbDescStats;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in re.findall(r"int(?:32|64)_t ([^;]+);", body) for n in decl.split(",")]
    assert names == [n for n, _ in YdMapDbDescStats._fields_] and C.sizeof(YdMapDbDescStats) == 80
    assert C.sizeof(YdMapDbRowStats) == 56 and C.sizeof(YdMapDbStats) == 72     # the older two keep their layouts
    for name in ("BAD 1", "NO_DESCRIPTORS 2", "VIEW_OUT_OF_RANGE 3", "UPDATED 0"):
        assert re.search(r"#define YDORB_MAPDESC_" + name.replace(" ", r" +"), hdr), name


def test_descriptor_adapter_typechecks():
    """enableDescriptors, touchDescriptors, computeDistinctiveDescriptors and verifyDescriptors of include/ydorb/mapMirror.hpp against
    declarations of the KeyFrame / MapPoint members they use."""
    H = os.path.join(ROOT, "tests", "cpu_harness")
    subprocess.check_call(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-I" + os.path.join(H, "mock"), os.path.join(H, "mapdesc_syntax_check.cpp")])
