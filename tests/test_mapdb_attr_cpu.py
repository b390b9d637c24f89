"""The resident table's point attributes without a GPU: the sanitized stand-alone check of ydorbslam_amd/csrc/mapdb_attr_host.h
(validation, coalescing per slot and per group, the clear record of an erased point, delta packing, the seeded sequence against a naive
model across two growths of the point table; tests/cpu_harness/mapdb_attr_check.cpp), what the six new C entries do on a machine with
no device, and the layouts the Python mirror and the header share.  The program is its own process: nothing is loaded into this one
under a sanitizer."""
import ctypes as C
import os
import re
import subprocess

import pytest

import mapdb_attr_support as R
from mapmaint_support import ROOT


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mapdbattr") / "mapdb_attr_check")
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


def test_attr_check_runs_clean_under_the_sanitizers(report):
    cases = [ln for ln in report if not ln.startswith("trace ")]
    assert cases[-1] == "0 failed" and len(cases) == 37 and not any("FAILED" in ln or "MISMATCH" in ln for ln in report)


def test_every_validation_message(report):
    for name, text in (("not enabled: set_point_attributes is refused", "point attributes are not enabled"),
                       ("negative n", "negative number of point slots: -1"), ("null slots with n > 0", "null slots"),
                       ("both groups null", "null geometry group and null desc"),
                       ("a partial geometry group: normal missing", "all three or none"),
                       ("a partial geometry group: min_distance missing", "all three or none"),
                       ("a partial geometry group: max_distance missing", "all three or none"),
                       ("slot past n_points", "slots[1]: point slot 40 outside 0..39"), ("negative slot", "slots[0]: point slot -1 outside 0..39"),
                       ("query slot past n_points", "point_slots[1]: point slot 40 outside 0..39")):
        assert text in _case(report, name)


def test_coalescing_clear_records_and_upload_accounting(report):
    for name in ("not enabled: the stats are all zero", "not enabled: an erased point stages nothing", "enable twice is fine",
                 "a rejected call stages nothing", "n == 0 with a group given", "staged points count: a slot staged and not yet synced",
                 "the first sync carries two records of 64 bytes", "nothing staged: last_attr_sync_bytes == 0",
                 "a slot never set reads as flags 0 and zero values", "coalescing: a slot set three times yields one record",
                 "coalescing: each group keeps its last value", "a null geometry group leaves it and its flag alone",
                 "a null desc leaves the descriptor and its flag alone", "the record names its groups and lies in the 64-byte format",
                 "an erased point stages one clear record", "an erased point reads as no attributes",
                 "the slot reused for a new point still reads as no attributes", "a set staged before the erase of the same interval is dropped",
                 "a set staged after the erase of the same interval stays", "... and the clear still zeroes the group the set does not name",
                 "set_points of a live point clears nothing", "clear drops what is staged and keeps capacity and counters"):
        _case(report, name)


def test_the_seeded_sequence_equals_the_model_across_two_growths(report):
    for name in ("sequence: every sync equals the model", "sequence: the arena grew with the point table, twice",
                 "sequence: one growth came with no attribute staged", "sequence: points with attributes were erased, and sets followed erases"):
        _case(report, name)
    trace = R.parse_trace(ln for ln in report if ln.startswith("trace "))
    assert len(trace) == 40 and trace[0]["capacity"] == R.SEQUENCE_CAPACITIES[0] and trace[-1]["capacity"] == 4 * R.SEQUENCE_CAPACITIES[0]
    assert [t["growths"] for t in trace] == sorted(t["growths"] for t in trace) and trace[-1]["growths"] == 2
    assert all(t["last_attr_sync_bytes"] == 64 * t["last_attr_sync_records"] for t in trace)
    assert trace[23]["last_attr_sync_records"] == 0 and trace[23]["capacity"] > trace[22]["capacity"]


def test_the_library_exports_the_new_entries_and_refuses_a_null_handle():
    import ydorbslam_amd as y
    L = y.lib()
    one = (C.c_int32 * 2)(0, 0)
    f = (C.c_float * 3)()
    row, st = (C.c_uint8 * 32)(), C.c_uint8(0)
    assert L.ydorb_mapdb_enable_attributes(None) == -1 and b"null handle" in L.ydorb_last_error()
    assert L.ydorb_mapdb_set_point_attributes(None, one, 1, f, f, f, row) == -1 and b"null handle" in L.ydorb_last_error()
    assert L.ydorb_mapdb_export_attributes(None, f, f, f, row, C.byref(st)) == -1 and b"null handle" in L.ydorb_last_error()
    assert L.ydorb_mapdb_attr_stats(None, None) == -1 and b"null handle or stats" in L.ydorb_last_error()
    assert L.ydorb_mapdb_search_local_points(None, None, None, None, one, 1, C.byref(st), 3.0, 0.8, None, None, None, None, None, None) == -1
    assert b"null argument" in L.ydorb_last_error()
    assert L.ydorb_mapdb_frustum_cull(None, None, -1, one, one, row, None, row, None) == -1 and b"negative number of views" in L.ydorb_last_error()
    assert L.ydorb_mapdb_frustum_cull(None, None, 0, None, one, row, None, row, None) == -1 and b"null list_start" in L.ydorb_last_error()
    rc = L.ydorb_mapdb_frustum_cull(None, None, 0, one, None, None, None, None, None)
    if L.ydorb_device_count() == 0:
        assert rc == -2                                                        # YDORB_ERR_NO_DEVICE: there is no CPU fallback
    else:
        assert rc == -1 and b"null handle" in L.ydorb_last_error()


def test_python_mirror_and_header_agree_on_the_attr_stats_layout():
    from ydorbslam_amd._lib import YdMapDbAttrStats, YdMapDbDescStats, YdMapDbRowStats, YdMapDbStats
    hdr = open(os.path.join(ROOT, "include", "ydorb", "c_api.h")).read()
    body = hdr[hdr.index("typedef struct YdMapDbAttrStats {"):hdr.index("} YdMapDbAttrStats;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in re.findall(r"int(?:32|64)_t ([^;]+);", body) for n in decl.split(",")]
    assert names == [n for n, _ in YdMapDbAttrStats._fields_] and C.sizeof(YdMapDbAttrStats) == 40
    assert C.sizeof(YdMapDbDescStats) == 80 and C.sizeof(YdMapDbRowStats) == 56 and C.sizeof(YdMapDbStats) == 72   # the older three keep their layouts
    assert re.search(r"#define YDORB_FRUSTUM_NO_ATTRIBUTES +7", hdr)
    for name, value in (("IN_VIEW", 0), ("SKIPPED", 1), ("BEHIND", 2), ("OUT_U", 3), ("OUT_V", 4), ("DISTANCE", 5), ("VIEW_ANGLE", 6)):
        assert re.search(r"#define YDORB_FRUSTUM_%s +%d\b" % (name, value), hdr), name       # the existing codes keep their values
