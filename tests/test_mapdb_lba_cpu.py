"""ydorb_mapdb_local_ba_graph without a GPU: the sanitized stand-alone check of ydorbslam_amd/csrc/mapdb_lba_host.h (every refusal, "a
refused call changes nothing", the result layout, the host execution against a std::map model on seeded tables;
tests/cpu_harness/mapdb_lba_check.cpp), what the new C entries do on a machine with no device, the layouts, and the conditions the
scenes of tests/mapdb_lba_support.py must meet, proved on the CPU reference alone so that no GPU test passes vacuously.
The program is its own process: nothing is loaded into this one under a sanitizer."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mapdb_lba_support as S
from mapmaint_support import ROOT


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mapdblba") / "mapdb_lba_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", S.CHECK_SRC, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    return r.stdout.splitlines()


@pytest.fixture(scope="module")
def default():
    s = S.Scene()
    return s, S.ref_graph(s.tables(), s.kf_slots)


def _case(report, name):
    hits = [ln for ln in report if ln.startswith(name)]
    assert len(hits) == 1 and " ok" in hits[0] and "FAILED" not in hits[0], (name, hits)
    return hits[0]


def test_lba_check_runs_clean_under_the_sanitizers(report):
    assert report[-1] == "0 failed" and not any("FAILED" in ln or "MISMATCH" in ln for ln in report)
    assert "compared 120 graphs" in report


def test_every_refusal_names_the_first_offender(report):
    for name, text in (("null out", "null out"), ("negative n_kf", "negative number of keyframe slots: -1"), ("null kf_slots", "null kf_slots"),
                       ("null inv_level_sigma2", "null inv_level_sigma2"),
                       ("features not enabled", "keyframe features are not enabled: call ydorb_mapdb_enable_features first"),
                       ("a slot outside 0..n_keyframes-1", "kf_slots[1]: keyframe slot 8 outside 0..7"),
                       ("a negative slot", "kf_slots[0]: keyframe slot -1 outside 0..7"),
                       ("a slot repeated in kf_slots", "kf_slots[3]: keyframe slot 1 is named twice")):
        assert text in _case(report, name)
    for name in ("a valid list", "n_kf == 0 with null kf_slots", "the result layout: aligned, the poses behind what the device writes"):
        _case(report, name)


def test_the_host_execution_equals_the_model_and_meets_every_path(report):
    for name in ("sequence: every graph equals the model's, bit for bit", "sequence: a refused call in between changes nothing",
                 "sequence: views of culled keyframes were skipped", "sequence: a view past its keyframe's features was met",
                 "sequence: a local point without an edge was met", "sequence: a fixed keyframe first met at a point rank >= 64",
                 "sequence: the view pool was repacked between two graphs"):
        _case(report, name)


def test_entries_without_a_device_bad_arguments_first():
    import ydorbslam_amd as y
    L = y.lib()
    assert L.ydorb_mapdb_lba_stats(None, None) == -1 and b"null handle or stats" in L.ydorb_last_error()
    assert L.ydorb_mapdb_lba_set_profiling(None, 1) == -1 and b"null handle" in L.ydorb_last_error()
    rc = L.ydorb_mapdb_local_ba_graph(None, None, 0, None, None)
    assert rc in (-1, -2) and (rc == -2 or b"null handle" in L.ydorb_last_error())   # no device: that is said first, there is no CPU path


def test_python_mirror_and_header_agree_on_the_layouts():
    from ydorbslam_amd._lib import YdBaProblem, YdLocalBaGraph, YdMapDbLbaStats
    hdr = open(os.path.join(ROOT, "include", "ydorb", "c_api.h")).read()

    def fields(name, types):
        body = hdr[hdr.index("typedef struct %s {" % name):hdr.index("} %s;" % name)]
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return [n.strip() for decl in re.findall(r"(?:%s)\*? ([^;]+);" % types, body) for n in decl.split(",")]
    assert fields("YdMapDbLbaStats", "int64_t|double") == [n for n, _ in YdMapDbLbaStats._fields_] and C.sizeof(YdMapDbLbaStats) == 72 + 32
    assert fields("YdLocalBaGraph", "YdBaProblem|int32_t|const int32_t|const uint8_t") == [n for n, _ in YdLocalBaGraph._fields_]
    assert C.sizeof(YdLocalBaGraph) == C.sizeof(YdBaProblem) + 8 + 5 * 8
    for name, value in (("SKIPPED_VIEWS", S.SKIPPED_VIEWS), ("VIEW_OUT_OF_RANGE", S.VIEW_OUT_OF_RANGE), ("NO_EDGES", S.NO_EDGES)):
        assert re.search(r"#define YDORB_LBA_POINT_%s +%d\b" % (name, value), hdr), name


def test_resident_overload_and_mirror_method_typecheck():
    """localBundleAdjustImpl<Frame>(mirror, ...) of optimizer.hpp and MapMirror::localBaGraph against mock declarations of the reference's
    members; the existing syntax checks stay as they are."""
    H = os.path.join(ROOT, "tests", "cpu_harness")
    subprocess.check_call(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-I" + os.path.join(H, "mock"), "-I" + os.path.join(H, "mockrt"),
                           os.path.join(H, "localba_resident_syntax_check.cpp")])


# ------------------------------------------------------------------------------------------------------------ the scenes
def test_the_default_scene_has_its_sizes(default):
    s, g = default
    n = len(g["point_slot"])
    print("local points", n, "edges", len(g["edge_pose"]), "fixed", g["n_fixed"])
    assert s.n_local == 6 and 600 <= n <= 800 and n > 2 * 256                      # more than two 256-lane workgroups in every scan
    assert all(len(s.rows[k]) == 300 for k in range(6))
    null = np.mean([np.mean(s.rows[k] < 0) for k in range(6)])
    assert 0.15 <= null <= 0.35, null                                             # about a quarter of the row entries are null
    lens = np.array([len(v) for v in s.views])
    assert lens.max() == 70 and lens[5] == 70 and sorted(set(lens) - {0, 70}) == list(range(1, 13))
    in_rows = np.unique(np.concatenate([s.rows[k][s.rows[k] >= 0] for k in range(6)]))
    assert s.bad[in_rows].sum() >= 5 and not np.isin(np.flatnonzero(s.bad), g["point_slot"]).any()   # bad points lie in rows and are left out
    mono = [bool((f[1] < 0).all()) for f in s.feats if len(f[0])]
    assert any(mono) and not all(mono)
    assert set(np.unique(np.concatenate([f[0]["octave"] for f in s.feats]))) == set(range(8))
    assert (g["edge_meas"][:, 2] == -1.0).any() and (g["edge_meas"][:, 2] >= 0).any()


def test_the_default_scene_meets_the_conditions_of_the_gpu_tests(default):
    s, g = default
    first = S.first_occurrence(g)
    assert g["n_fixed"] >= 5 and len(first) == g["n_fixed"]
    ranks = sorted(r for r, _ in first.values())
    assert sum(r >= 256 for r in ranks) >= 2 and sum(r >= 512 for r in ranks) >= 1, ranks[-5:]
    big = int(np.flatnonzero(g["point_slot"] == 5)[0])                              # the 70-view point is local ...
    pos_in_span = {int(k): j for j, (k, _) in enumerate(s.views[5])}
    assert any(r == big and pos_in_span[k] >= 64 for k, (r, _) in first.items())  # at view position >= 64
    assert (g["point_status"] & S.SKIPPED_VIEWS).any()                            # an unusable keyframe observed by a local point
    assert (g["point_status"] == S.NO_EDGES).sum() >= 1                           # the point nobody sees
    # a local keyframe observed by a point first reached through another keyframe's row
    row_of_first = {int(p): k for k in reversed(range(6)) for p in s.rows[k][s.rows[k] >= 0]}
    assert any(g["pose_kf"][g["edge_pose"][e]] != row_of_first[int(g["point_slot"][g["edge_point"][e]])] and g["edge_pose"][e] < 6
               for e in range(len(g["edge_pose"])))
    fixed = g["pose_kf"][6:]
    assert not np.array_equal(fixed, np.sort(fixed))                              # the fixed order is not ascending-slot order
    order = np.lexsort((g["edge_point"], g["edge_pose"]))
    assert not np.array_equal(order, np.arange(len(order)))                       # the edge order is not a sort by (pose, point)


def test_the_reference_agrees_with_the_dict_statement(default):
    s, g = default
    S.same_graph(g, S.dict_graph(s.tables(), s.kf_slots))
    for kf in ([3], [], [5, 0, 2], list(range(6, 20)), [45, 1]):
        S.same_graph(S.ref_graph(s.tables(), kf), S.dict_graph(s.tables(), kf))


def test_the_swap_scene_makes_fixed_keyframes_local_and_local_ones_fixed(default):
    s, g = default
    a, b = s.kf_slots, g["pose_kf"][6:12]
    gb = S.ref_graph(s.tables(), b)
    assert np.isin(a, gb["pose_kf"][gb["n_local"]:]).sum() >= 3 and gb["n_fixed"] >= 5   # A's local keyframes are fixed in B


def test_the_solver_scene_has_the_sizes_of_the_smallest_interesting_solve():
    s = S.solver_scene()[0]
    g = S.ref_graph(s.tables(), s.kf_slots)
    assert g["n_local"] == 8 and 4 <= g["n_fixed"] <= 6 and 250 <= len(g["point_slot"]) <= 320
    assert (g["edge_meas"][:, 2] < 0).any() and (g["edge_meas"][:, 2] >= 0).any()
    S.same_graph(g, S.dict_graph(s.tables(), s.kf_slots))
