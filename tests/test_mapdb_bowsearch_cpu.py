"""The batched BoW searches over the resident table without a GPU: the sanitized stand-alone check of
ydorbslam_amd/csrc/mapdb_bowsearch_host.h (every refusal of the frame validation, bowSearchOnHost against a std::map-based second
statement over a seeded sequence that passes rows, features, blocks and BoW spans through their host halves;
tests/cpu_harness/mapdb_bowsearch_check.cpp), what the new C entries do on a machine with no device, the header's constants, and the
conditions the scenes of tests/mapdb_bowsearch_support.py must meet, proved on the reference alone: every GPU comparison in
tests/test_mapdb_bowsearch_gpu.py is exact, so what it can tell apart is decided here.
The program is its own process: nothing is loaded into this one under a sanitizer."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mapdb_bowsearch_support as B
from mapmaint_support import ROOT


# ------------------------------------------------------------------------------------------------------------ the check program
@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mapdbbowsearch") / "mapdb_bowsearch_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", B.CHECK_SRC, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    return r.stdout.splitlines()


def _case(report, name):
    hits = [ln for ln in report if ln.startswith(name)]
    assert len(hits) == 1 and " ok" in hits[0] and "FAILED" not in hits[0], (name, hits)
    return hits[0]


def test_bowsearch_check_runs_clean_under_the_sanitizers(report):
    assert report[-1] == "0 failed" and not any("FAILED" in ln for ln in report)


def test_every_refusal_of_the_frame_names_the_first_offender(report):
    for name, text in (("null frame", "null frame"), ("n of -1", "frame: n -1 outside 0..65535"), ("n of 65536", "frame: n 65536 outside 0..65535"),
                       ("null kps", "frame: null kps or desc"), ("null desc", "frame: null kps or desc"),
                       ("negative n_nodes", "frame: negative number of nodes: -2"), ("null node_start", "frame: null node_start"),
                       ("node_start[0] != 0", "frame: node_start[0] is 1, not 0"), ("node_start decreases", "frame: node_start decreases at 2"),
                       ("null node_ids", "frame: null node_ids"), ("node ids that repeat", "frame: node id 7 after 7"),
                       ("node ids that decrease", "frame: node id 5 after 7"), ("null feat", "frame: null feat"),
                       ("a feature index of n", "frame: entry 3: feature index 4 outside 0..3"),
                       ("a feature index of -1", "frame: entry 1: feature index -1 outside 0..3")):
        assert text in _case(report, name)
    for name in ("a frame of 65535 features", "an empty frame", "a frame without nodes", "null valid is every feature", "a node id of 2^32 - 1"):
        _case(report, name)


def test_flattening_prefix_sums_and_the_search_against_the_second_statement(report):
    for name in ("flatten: map order", "query starts skip the unusable", "query starts past INT32_MAX", "good map point: the three clauses",
                 "sequence: every search equals the second statement", "sequence: the row and BoW pools repacked", "sequence: matches in both modes",
                 "sequence: a bad point, a never-set slot and an invalid frame feature each decided a query",
                 "sequence: the rotation histogram culled a match"):
        _case(report, name)


# ------------------------------------------------------------------------------------------------------------ the entries, no device
def test_entries_without_a_device_bad_arguments_first():
    import ydorbslam_amd as y
    L = y.lib()
    assert L.ydorb_mapdb_search_by_bow_keyframes(None, None, 0, None, 0, 0.6, 0, 0, None, None, None, None) == -1 and b"null handle" in L.ydorb_last_error()
    assert L.ydorb_mapdb_search_by_bow_frame(None, None, None, 0, None, 0.6, 0, None, None, None, None) == -1 and b"null handle" in L.ydorb_last_error()
    assert L.ydorb_matcher_bow_search_stats(None, None) == -1 and b"null handle or stats" in L.ydorb_last_error()
    from ydorbslam_amd._lib import YdBowSearchStats
    assert C.sizeof(YdBowSearchStats) == 7 * 8 + 4 + 3 * 4


def test_the_header_has_the_pair_status_values_of_the_neighbour_status():
    hdr = open(os.path.join(ROOT, "include", "ydorb", "c_api.h")).read()
    for name, value in B.PAIR_STATUS.items():
        assert re.search(r"#define YDORB_BOW_PAIR_%s +%d\b" % (name.upper(), value), hdr), name
        assert re.search(r"#define YDORB_CREATE_NB_%s +%d\b" % (name.upper(), value), hdr), name
    src = open(os.path.join(ROOT, "ydorbslam_amd", "csrc", "match_kernels.hip.h")).read()
    assert re.search(r"kResolveWindow = %d\b" % B.RESOLVE_WINDOW, src)
    src = open(os.path.join(ROOT, "ydorbslam_amd", "csrc", "orb_matcher.hip")).read()
    assert re.search(r"triPoolPerNb = 1u << 14\b", src) and B.POOL_PER_PAIR == 1 << 14


def test_resident_overloads_and_mirror_methods_typecheck():
    """searchByBowInTwoKeyFrames / searchByBowInKeyFrameAndFrame over a mirror, trackReferenceKeyFrameSearchImpl and the two MapMirror
    methods against mock declarations of the reference's members; the existing syntax checks stay as they are."""
    H = os.path.join(ROOT, "tests", "cpu_harness")
    subprocess.check_call(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-I" + os.path.join(H, "mock"), os.path.join(H, "bowsearch_resident_syntax_check.cpp")])


# ------------------------------------------------------------------------------------------------------------ the scenes
def _pairs(s):
    """(mode, candidate slot, keyword arguments of reference / analyse) of every pair of a scene, both forms."""
    for c in s.slots[1:]:
        yield 4, c, dict(first=s.slots[0])
        yield 3, c, dict(frame=s.frame)


@pytest.fixture(scope="module")
def analysed(oracle_lib):
    """analyse() of every pair of every scene at ratio 0.6, each held to the oracle first."""
    out = {}
    for name in B.SCENES:
        s = B.scene(name)
        arrays = s.host_arrays()
        for mode, c, kw in _pairs(s):
            a = B.analyse(arrays, mode, c, 0.6, **kw)
            want = B.reference(oracle_lib, arrays, mode, [c], 0.6, False, **kw)
            assert np.array_equal(a["matched"], want["matched"][0]) and a["n_matches"] == want["n_matches"][0], (name, mode, c)
            out[name, mode, c] = a
    return out


def test_every_usable_pair_has_at_least_30_matches_without_the_orientation_check(oracle_lib):
    for name in B.SCENES:
        s = B.scene(name)
        arrays = s.host_arrays()
        for ratio in B.RATIOS:
            for mode, c, kw in _pairs(s):
                r = B.reference(oracle_lib, arrays, mode, [c], ratio, False, **kw)
                if name == "disjoint" and c == s.slots[2]:
                    assert r["n_matches"][0] == 0 and (r["matched"] == -1).all()
                else:
                    assert r["n_matches"][0] >= 30, (name, mode, c, ratio, r["n_matches"])


def test_the_rotation_histogram_takes_matches_away(oracle_lib):
    s = B.default_scene()
    arrays = s.host_arrays()
    for mode in (4, 3):
        lost = 0
        for m, c, kw in _pairs(s):
            if m == mode:
                off, on = (B.reference(oracle_lib, arrays, mode, [c], 0.6, flag, **kw) for flag in (False, True))
                assert on["n_matches"][0] <= off["n_matches"][0]
                lost += int(off["n_matches"][0] - on["n_matches"][0])
        assert lost >= 1, mode


def test_the_ratios_differ(oracle_lib):
    s = B.default_scene()
    arrays = s.host_arrays()
    for mode, c, kw in list(_pairs(s))[:2]:
        n = [int(B.reference(oracle_lib, arrays, mode, [c], ratio, False, **kw)["n_matches"][0]) for ratio in B.RATIOS]
        assert n[0] < n[2], (mode, n)


def test_ratio_taken_bad_and_never_set_each_decide_something(analysed):
    for mode in (4, 3):
        d = [a for (name, m, c), a in analysed.items() if name == "default" and m == mode]
        assert sum(a["ratio_only"] for a in d) >= 1, mode      # rejected by the ratio test alone
        assert sum(a["taken"] for a in d) >= 1, mode           # a resolve that ignored `taken` would answer differently
        assert sum(a["emptied"] for a in d) >= 1, mode         # a query emptied only by a bad point or a never-set slot
    assert sum(a["dropped"] for (name, m, c), a in analysed.items() if name == "default" and m == 4) >= 1   # a candidate dropped for the same reason
    s = B.default_scene()
    bad = s.bad
    for k in s.kfs:                                            # both kinds occur in every row: flagged bad, and never set
        named = k["row"][k["row"] >= 0]
        assert np.isin(named, s.never).any() and (bad[named][~np.isin(named, s.never)] == 1).any()
    assert 0.6 < np.mean(np.concatenate([k["row"] for k in s.kfs]) >= 0) < 0.8 and 0.05 < bad.mean() < 0.2
    assert [len(k["row"]) for k in s.kfs] == [300, 307, 314, 321, 328] and len(s.frame["kps"]) == 303
    assert s.frame["valid"].min() == 0 and s.frame["valid"].max() == 1


def test_the_bucket_scene_has_its_three_sizes_on_every_b_side(analysed):
    s = B.scene("buckets")
    for side in s.kfs[1:] + [s.frame]:
        ids, counts = np.unique(side["bow"][:, 0], return_counts=True)
        size = dict(zip(ids.tolist(), counts.tolist()))
        assert (size[10], size[20], size[30]) == (130, 64, 65)
    nodes0 = s.kfs[0]["nodes"]
    for node in (10, 20, 30):                                  # ... and the first keyframe has matches in each
        for c in s.slots[1:]:
            assert ((analysed["buckets", 4, c]["matched"] >= 0) & (nodes0 == node)).sum() >= 3, node


def test_the_end_nodes_lie_below_and_above_every_node_of_the_b_side():
    s = B.scene("ends")
    a4, a3 = s.kfs[0]["bow"][:, 0], [k["bow"][:, 0] for k in s.kfs[1:]]
    assert all(a4.min() < b.min() and a4.max() > b.max() for b in a3)                      # mode 4: A = the first keyframe, B = a candidate
    fb = s.frame["bow"][:, 0]
    assert all(a.min() < fb.min() and a.max() > fb.max() for a in a3)                      # mode 3: A = a candidate, B = the frame


def test_the_600_feature_scene_has_matches_on_both_sides_of_the_resolve_window(analysed):
    s = B.scene("six_hundred")
    assert len(s.kfs[0]["bow"]) == 600 > B.RESOLVE_WINDOW and all(len(k["bow"]) > B.RESOLVE_WINDOW for k in s.kfs[1:])
    q_of = {int(f): q for q, f in enumerate(s.kfs[0]["bow"][:, 1])}
    for c in s.slots[1:]:
        q = [q_of[int(i)] for i in np.flatnonzero(analysed["six_hundred", 4, c]["matched"] >= 0)]
        assert min(q) < B.RESOLVE_WINDOW <= max(q)


def test_the_one_node_scene_asks_for_more_records_than_a_fresh_pool_holds(analysed):
    s = B.scene("one_node")
    assert any(analysed["one_node", 4, c]["records"] > B.POOL_PER_PAIR for c in s.slots[1:])
    assert any(analysed["one_node", 3, c]["records"] > B.POOL_PER_PAIR for c in s.slots[1:])
    assert all(analysed["one_node", m, c]["reserved"] >= analysed["one_node", m, c]["records"] for m in (3, 4) for c in s.slots[1:])


def test_the_other_scenes_fit_a_fresh_pool(analysed):
    assert all(a["records"] <= a["reserved"] <= B.POOL_PER_PAIR for (name, m, c), a in analysed.items() if name != "one_node")


def test_the_disjoint_candidate_shares_no_node(analysed):
    s = B.scene("disjoint")
    c = s.slots[2]
    assert not analysed["disjoint", 4, c]["common"] and not analysed["disjoint", 3, c]["common"]
    assert all(analysed["disjoint", m, o]["common"] for m in (3, 4) for o in s.slots[1:] if o != c)
