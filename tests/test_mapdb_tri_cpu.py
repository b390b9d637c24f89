"""The resident table's BoW feature vectors and createNewMapPoints on the table without a GPU: the sanitized stand-alone check of
ydorbslam_amd/csrc/mapdb_bow_host.h (every refusal, coalescing, erase, clear, delta packing, the pool policy, the seeded sequence against
a naive model with every delta executed on host arrays; tests/cpu_harness/mapdb_bow_check.cpp), what the new C entries do on a machine
with no device, the layouts, and the conditions the scenes of tests/mapdb_tri_support.py must meet, proved on the CPU reference alone.
The program is its own process: nothing is loaded into this one under a sanitizer."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mapdb_tri_support as T
from mapmaint_support import ROOT


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mapdbbow") / "mapdb_bow_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", T.CHECK_SRC, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    return r.stdout.splitlines()


def _case(report, name):
    hits = [ln for ln in report if ln.startswith(name)]
    assert len(hits) == 1 and " ok" in hits[0] and "FAILED" not in hits[0], (name, hits)
    return hits[0]


def test_bow_check_runs_clean_under_the_sanitizers(report):
    cases = [ln for ln in report if not ln.startswith("trace ")]
    assert cases[-1] == "0 failed" and len(cases) == 43 and not any("FAILED" in ln or "MISMATCH" in ln for ln in report)


def test_every_refusal_names_the_first_offender(report):
    for name, text in (("set before enable", "keyframe BoW feature vectors are not enabled: call ydorb_mapdb_enable_bow first"),
                       ("bow_start[0] != 0", "bow_start[0] is 1, not 0"), ("bow_start decreases", "bow_start decreases at 2"),
                       ("negative keyframe slot", "kf_slots[1]: negative keyframe slot -3"), ("null bow_start", "null bow_start"),
                       ("null kf_slots", "null kf_slots"), ("null node_id", "null node_id or feat"), ("null feat", "null node_id or feat"),
                       ("negative n", "negative number of keyframe slots: -1"),
                       ("a span longer than 65 535", "a span of 65536 entries, more than 65535"),
                       ("node ids that decrease inside a span", "entry 2: node id 7 after 9"),
                       ("a node id of 2^31", "entry 3: node id 2147483648 outside 0..2147483647"),
                       ("a feature index of 65535", "entry 1: feature index 65535 outside 0..65534"),
                       ("a feature index of -1", "entry 4: feature index -1 outside 0..65534"),
                       ("a feature index that repeats inside one span", "entry 2: feature index 4 repeats inside its span"),
                       ("a pool past INT32_MAX entries", "2147483648 entries, past INT32_MAX")):
        assert text in _case(report, name)
    for name in ("a span of 65 535", "a pool of INT32_MAX entries", "the largest node id, 2^31 - 1", "node ids may fall from one span to the next",
                 "a feature index may repeat across spans", "the refused calls staged nothing", "a refused set_keyframe_bow stages nothing",
                 "... nor when a later entry is malformed", "... and nothing is dirty", "... and the relation is what it was"):
        _case(report, name)


def test_coalescing_erase_clear_and_upload_accounting(report):
    for name in ("a handle that never enables counts nothing", "stats count what is staged", "a slot never set has no feature vector",
                 "delta payload offsets are 16-byte aligned", "the delta carries no entry records", "nothing staged: last_bow_sync_bytes == 0",
                 "coalescing: a vector set three times costs the last span only", "coalescing: a slot named twice in one call keeps its last span",
                 "a span of length 0 erases the feature vector", "clear empties the relation and keeps capacities and counters", "clear, then reuse"):
        _case(report, name)


def test_the_seeded_sequence_equals_the_model_and_meets_every_path(report):
    for name in ("sequence: every sync equals the model", "sequence: a repack that kept the capacity", "sequence: a repack that grew the capacity",
                 "sequence: the headers grew past the initial keyframe capacity"):
        _case(report, name)
    trace = T.parse_trace(ln for ln in report if ln.startswith("trace "))
    assert len(trace) == 44 and trace[-1]["repacks_kept"] >= 1 and trace[-1]["repacks_grown"] >= 2
    assert min(t["n_entries"] for t in trace) < trace[0]["n_entries"] * 0.5          # most keyframes were culled at once
    assert trace[29]["n_entries"] > trace[11]["n_entries"] * 2                       # ... and came back
    assert trace[30]["pool_used"] == trace[30]["n_entries"]                          # the clear: the pool holds what was set after it, no garbage
    assert all(t["pool_used"] <= t["pool_capacity"] and t["n_entries"] <= t["pool_used"] for t in trace)


def test_entries_without_a_device_bad_arguments_first():
    import ydorbslam_amd as y
    L = y.lib()
    assert L.ydorb_mapdb_enable_bow(None) == -1 and b"null handle" in L.ydorb_last_error()
    assert L.ydorb_mapdb_set_keyframe_bow(None, None, 0, None, None, None) == -1 and b"null handle" in L.ydorb_last_error()
    assert L.ydorb_mapdb_export_bow(None, None, None, None) == -1 and b"null handle" in L.ydorb_last_error()
    assert L.ydorb_mapdb_bow_stats(None, None) == -1 and b"null handle or stats" in L.ydorb_last_error()
    assert L.ydorb_mapdb_create_new_points(None, None, None, None, 0, 0, 0, None, None, None, None, None, None) == -1 and b"null handle" in L.ydorb_last_error()
    n_calls = C.c_int32(0)
    assert L.ydorb_matcher_create_points_times(None, None, C.byref(n_calls)) == -1


def test_python_mirror_and_header_agree_on_the_layouts():
    from ydorbslam_amd._lib import YdCreateNeighbour, YdCreateView, YdMapDbAttrStats, YdMapDbBowStats, YdMapDbDescStats, YdMapDbFeatStats, YdMapDbRowStats, YdMapDbStats
    hdr = open(os.path.join(ROOT, "include", "ydorb", "c_api.h")).read()

    def fields(name, types):
        body = hdr[hdr.index("typedef struct %s {" % name):hdr.index("} %s;" % name)]
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return [re.sub(r"\[\d+\]", "", n).strip() for decl in re.findall(r"(?:%s)\*? ([^;]+);" % types, body) for n in decl.split(",")]
    assert fields("YdMapDbBowStats", "int32_t|int64_t") == [n for n, _ in YdMapDbBowStats._fields_] and C.sizeof(YdMapDbBowStats) == 56
    assert fields("YdCreateView", "int32_t|const float|float") == [n for n, _ in YdCreateView._fields_] and C.sizeof(YdCreateView) == 16 + 4 * (24 + 8 + 16) + 8
    assert fields("YdCreateNeighbour", "YdCreateView|float") == [n for n, _ in YdCreateNeighbour._fields_]
    assert C.sizeof(YdCreateNeighbour) == C.sizeof(YdCreateView) + 4 * 12
    assert (C.sizeof(YdMapDbStats), C.sizeof(YdMapDbRowStats), C.sizeof(YdMapDbDescStats), C.sizeof(YdMapDbAttrStats), C.sizeof(YdMapDbFeatStats)) == (72, 56, 80, 40, 56)
    assert re.search(r"#define YDORB_TRI_UNMATCHED +%d\b" % T.UNMATCHED, hdr)
    for name, value in T.NB_STATUS.items():
        assert re.search(r"#define YDORB_CREATE_NB_%s +%d\b" % (name.upper(), value), hdr), name


# ------------------------------------------------------------------------------------------------------------ the scenes
def test_the_default_scene_meets_its_conditions(oracle_lib):
    """About 300 features, 4 neighbours, 12 nodes, a stereo / mono mix, map points on both sides; every neighbour matches at least 20 and
    accepts at least 5; the claims change a later neighbour's matches; a geometric rejection is matched again later."""
    s = T.default_scene()
    with_claims, _ = T.check_scene_conditions(s, oracle_lib)
    assert s.n == 300 and s.n_nb == 4 and len(np.unique(s.kfs[0]["nodes"])) == 12
    for k in s.kfs:
        v = k["view"]
        assert (v["right_x"] >= 0).any() and (v["right_x"] < 0).any() and (k["row"] >= 0).any() and (k["row"] < 0).any()
    assert len({len(k["row"]) for k in s.kfs}) == s.n_nb + 1                               # every keyframe has a feature count of its own
    assert len(set(np.unique(with_claims["status"] & 15)) - {0, T.UNMATCHED}) >= 1         # the geometry rejects some matches


def test_the_flag_forms_change_the_result(oracle_lib):
    s = T.default_scene()
    base = s.reference(oracle_lib)
    for kw in (dict(stereo_only=True), dict(check_orientation=True)):
        r = s.reference(oracle_lib, **kw)
        assert r["n_matches"].min() >= 5 and not np.array_equal(r["matched_second"], base["matched_second"]), kw


def test_the_bucket_scene_has_its_three_sizes_and_matches_in_each(oracle_lib):
    s = T.Scene(seed=6, nodes=T.bucket_nodes)
    for k in s.kfs:
        ids, counts = np.unique(k["nodes"][:300], return_counts=True)
        assert dict(zip(ids.tolist(), counts.tolist()))[10] == 130 and dict(zip(ids.tolist(), counts.tolist()))[20] == 64 and dict(zip(ids.tolist(), counts.tolist()))[30] == 65
    r = s.reference(oracle_lib)
    nodes0 = s.kfs[0]["nodes"]
    for node in (10, 20, 30):
        assert ((r["matched_second"] >= 0) & (nodes0 == node)[None, :]).sum() >= 5, node


def test_the_end_nodes_lie_outside_every_neighbour_span(oracle_lib):
    s = T.Scene(seed=7, nodes=T.end_nodes)
    lo, hi = s.kfs[0]["bow"][:, 0].min(), s.kfs[0]["bow"][:, 0].max()
    assert all(lo < k["bow"][:, 0].min() and hi > k["bow"][:, 0].max() for k in s.kfs[1:])
    assert (s.reference(oracle_lib)["n_matches"] >= 10).all()


def test_the_replay_scene_asks_for_more_records_than_a_fresh_pool_holds(oracle_lib):
    s = T.Scene(seed=8, n_nb=2, nodes=T.one_node)
    eligible = int((s.kfs[0]["row"] < 0).sum())
    assert all(eligible * len(k["row"]) > T.POOL_PER_NEIGHBOUR for k in s.kfs[1:])        # one bucket: every eligible feature meets every feature
    r, without = s.reference(oracle_lib), s.reference(oracle_lib, claims=False)
    assert (r["n_matches"] >= 20).all() and not np.array_equal(r["matched_second"][1], without["matched_second"][1])   # an attempt's stale claims would show
