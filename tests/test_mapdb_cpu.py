"""The resident map table without a GPU: the sanitized stand-alone check of ydorbslam_amd/csrc/mapdb_host.h (validation, coalescing,
delta packing, pool policy and the seeded state-machine sequence against a naive model, tests/cpu_harness/mapdb_host_check.cpp), that
of the pool policy on its own (ydorbslam_amd/csrc/span_pool.h, tests/cpu_harness/span_pool_check.cpp), what the C entries do on a
machine with no device, and the adapter's type check.  Each program is its own process: nothing is loaded into this one under a
sanitizer."""
import ctypes as C
import os
import subprocess

import pytest

import mapdb_support as D
from mapmaint_support import ROOT


def _sanitized_report(src, exe):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", src, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    return r.stdout.splitlines()


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    return _sanitized_report(D.CHECK_SRC, str(tmp_path_factory.mktemp("mapdb") / "mapdb_host_check"))


def _case(report, name):
    hits = [ln for ln in report if ln.startswith(name)]
    assert len(hits) == 1 and " ok" in hits[0] and "FAILED" not in hits[0], (name, hits)
    return hits[0]


def test_host_check_runs_clean_under_the_sanitizers(report):
    cases = [ln for ln in report if not ln.startswith("trace ")]
    assert cases[-1] == "0 failed" and len(cases) == 40 and not any("FAILED" in ln or "MISMATCH" in ln for ln in report)


def test_every_validation_message(report):
    for name, text in (("obs_start[0] != 0", "obs_start[0] is 1, not 0"), ("obs_start decreases", "obs_start decreases at 2"),
                       ("obs_kf out of range", "observation 1: keyframe slot 4 outside 0..3"), ("obs_kf negative", "keyframe slot -1"),
                       ("ref_kf out of range", "point 1: reference keyframe slot 4 outside 0..3"), ("negative point slot", "negative point slot -2"),
                       ("null obs_kf", "null obs_kf or obs_level"), ("null pos", "null slots, bad, ref_kf, ref_level or pos"),
                       ("null obs_start", "null obs_start"), ("negative n", "negative number of point slots: -1"),
                       ("set_positions past n_points", "point slot 3 outside 0..2"), ("set_positions null pos", "null slots or pos"),
                       ("set_centres negative slot", "negative keyframe slot -1"), ("set_centres null centre", "null kf_slots or centre"),
                       ("query slot past n_points", "point slot 3 outside 0..2"), ("query n_levels 9", "n_levels 9 outside 1..8"),
                       ("query null scale_factors", "null scale_factors"), ("query null outputs", "null output arrays"),
                       ("ref_level >= n_levels of an updated point", "reference level 7 of point slot 2 >= n_levels"),
                       ("query_kf out of range", "query_kf[0]: keyframe slot 4 outside 0..3"),
                       ("list entry out of range", "point index 3 outside the table of 3"),
                       ("a pool past INT32_MAX entries", "2147483648 observations, past INT32_MAX")):
        assert text in _case(report, name)


def test_coalescing_rejection_and_upload_accounting(report):
    for name in ("coalescing: three sets, the pool grows by the last span", "stats count the staged span", "a rejected set_points stages nothing",
                 "the rejected calls staged nothing", "nothing dirty: last_sync_bytes == 0", "a slot never set reads as bad and empty", "clear, then reuse",
                 "three touched spans: the same bytes at 100 and 10 000 points"):
        _case(report, name)


def test_the_seeded_sequence_equals_the_model_and_meets_every_path(report):
    for name in ("sequence: every sync equals the model", "sequence: a repack that kept the capacity", "sequence: a repack that grew the capacity",
                 "sequence: a point-table growth", "sequence: a keyframe-table growth"):
        _case(report, name)
    trace = D.parse_trace(ln for ln in report if ln.startswith("trace "))
    assert len(trace) == 49 and trace[0]["n_points"] == 600 and trace[0]["n_keyframes"] == 40
    last = trace[-1]
    assert min(last["repacks_kept"], last["repacks_grown"], last["point_table_growths"], last["keyframe_table_growths"]) >= 1
    assert last["n_points"] > 900 and min(t["n_observations"] for t in trace) < trace[0]["n_observations"] * 0.6      # half of the spans went empty once


def test_span_pool_check_runs_clean_under_the_sanitizers(tmp_path):
    """Every rule of span_pool.h at the smallest numbers at which it can go wrong: the case names are the rules."""
    report = _sanitized_report(os.path.join(ROOT, "tests", "cpu_harness", "span_pool_check.cpp"), str(tmp_path / "span_pool_check"))
    assert report[-1] == "0 failed" and len(report) == 37 and not any("FAILED" in ln for ln in report)
    for name in ("used + incoming == capacity: no repack, tail = used", "used + incoming == capacity + 1: repack, tail = survivors",
                 "capacity 8: need 4 keeps the capacity", "capacity 8: need 5 grows it to 10", "capacity 9: need 4 keeps the capacity",
                 "capacity 9: need 5 grows it to 10", "need 2^30 + 1: the capacity is INT32_MAX", "all live entries replaced: survivors 0, tail 0 on repack",
                 "nothing incoming with a full pool: no repack", "commit without a repack: no counter moves", "commit of a kept repack: live, used, one counter",
                 "commit of a grown repack: live, used, the other counter", "survivors in ascending slot order", "a replaced slot gets -1, adds nothing",
                 "a zero-length survivor shares the next slot's offset", "the last offset plus its length equals the survivors",
                 "table growth: needed <= capacity is unchanged", "table growth: capacity + 1 gives 2 x capacity",
                 "table growth: 3 x capacity gives 3 x capacity", "table growth: capacity 2^30 + 1 gives INT32_MAX", "a total of INT32_MAX passes",
                 "one slot named twice counts its last length only", "delta sections: 16-byte aligned"):
        _case(report, name)
    assert "the pool would hold 2147483648 observations, past INT32_MAX" in _case(report, "INT32_MAX + 1 observations")
    assert "the row pool would hold 2147483648 entries, past INT32_MAX" in _case(report, "INT32_MAX + 1 row entries")


def test_create_without_a_device_is_no_device_and_bad_arguments_come_first():
    import ydorbslam_amd as y
    L = y.lib()
    h = C.c_void_p()
    assert L.ydorb_mapdb_create(16, 16, 4, 64, C.byref(h)) == -1 and b"device 16 outside" in L.ydorb_last_error()
    assert L.ydorb_mapdb_create(0, -1, 4, 64, C.byref(h)) == -1 and b"negative capacity" in L.ydorb_last_error()
    assert L.ydorb_mapdb_create(0, 1, 1, 2 ** 31, C.byref(h)) == -1 and b"INT32_MAX" in L.ydorb_last_error()
    assert L.ydorb_mapdb_create(0, 1, 1, 1, None) == -1
    assert L.ydorb_mapdb_clear(None) == -1 and L.ydorb_mapdb_stats(None, None) == -1 and L.ydorb_mapdb_set_positions(None, None, 0, None) == -1
    L.ydorb_mapdb_destroy(None)
    rc = L.ydorb_mapdb_create(0, 16, 4, 64, C.byref(h))
    if L.ydorb_device_count() == 0:
        assert rc == -2 and not h                                              # YDORB_ERR_NO_DEVICE: there is no CPU fallback
        with pytest.raises(y.YdorbError, match="ydorb error -2"):
            y.MapDb()
    else:
        assert rc == 0 and h
        L.ydorb_mapdb_destroy(h)


def test_python_mirror_and_header_agree_on_the_stats_layout():
    from ydorbslam_amd._lib import YdMapDbStats
    hdr = open(os.path.join(ROOT, "include", "ydorb", "c_api.h")).read()
    body = hdr[hdr.index("typedef struct YdMapDbStats {"):hdr.index("} YdMapDbStats;")]
    import re
    names = [n.strip() for decl in re.findall(r"int(?:32|64)_t ([^;]+);", body) for n in decl.split(",")]
    assert names == [n for n, _ in YdMapDbStats._fields_] and C.sizeof(YdMapDbStats) == 72


def test_map_mirror_typechecks():
    """include/ydorb/mapMirror.hpp against declarations of the KeyFrame / MapPoint members it uses."""
    H = os.path.join(ROOT, "tests", "cpu_harness")
    subprocess.check_call(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-I" + os.path.join(H, "mock"), os.path.join(H, "mapmirror_syntax_check.cpp")])
