"""The resident table's keyframe features and the batched fuse search without a GPU: the sanitized stand-alone check of
ydorbslam_amd/csrc/mapdb_feat_host.h (validation, coalescing, erase, delta packing, the pool policy, the seeded sequence against a naive
model with every delta executed on host arrays; tests/cpu_harness/mapdb_feat_check.cpp), what the five new C entries do on a machine
with no device, and the CPU restatement of the query's pass 1 (tests/fuse_ref) against a literal numpy statement of the adapter's.  The
program is its own process: nothing is loaded into this one under a sanitizer."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mapdb_fuse_support as R
from mapmaint_support import ROOT


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mapdbfeat") / "mapdb_feat_check")
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


def test_feat_check_runs_clean_under_the_sanitizers(report):
    cases = [ln for ln in report if not ln.startswith("trace ")]
    assert cases[-1] == "0 failed" and len(cases) == 38 and not any("FAILED" in ln or "MISMATCH" in ln for ln in report)


def test_every_validation_message(report):
    for name, text in (("set before enable", "keyframe features are not enabled: call ydorb_mapdb_enable_features first"),
                       ("feat_start[0] != 0", "feat_start[0] is 1, not 0"), ("feat_start decreases", "feat_start decreases at 2"),
                       ("negative keyframe slot", "kf_slots[1]: negative keyframe slot -3"), ("null feat_start", "null feat_start"),
                       ("null kf_slots", "null kf_slots"), ("null kps", "null kps"), ("negative n", "negative number of keyframe slots: -1"),
                       ("octave 8", "feature 4: octave 8 outside 0..7"), ("octave -1", "feature 1: octave -1 outside 0..7"),
                       ("a span longer than 65 535", "a span of 65536 features, more than 65535"),
                       ("a pool past INT32_MAX features", "2147483648 features, past INT32_MAX")):
        assert text in _case(report, name)
    for name in ("a span of 65 535", "a pool of INT32_MAX features", "null right_x is accepted", "null right_x stores -1 for every feature"):
        _case(report, name)


def test_coalescing_rejection_erase_and_upload_accounting(report):
    for name in ("a handle that never enables counts nothing", "stats count what is staged", "a slot never set has no features",
                 "delta payload offsets are 16-byte aligned", "one span indexes both arrays", "nothing staged: last_feat_sync_bytes == 0",
                 "the rejected calls staged nothing", "a rejected set_keyframe_features stages nothing", "... nor when a later feature is malformed",
                 "... and nothing is dirty", "... and the relation is what it was", "coalescing: features set three times cost the last span only",
                 "coalescing: a slot named twice in one call keeps its last span", "a span of length 0 erases the features",
                 "clear empties the relation and keeps capacities and counters", "clear, then reuse"):
        _case(report, name)


def test_the_seeded_sequence_equals_the_model_and_meets_every_path(report):
    for name in ("sequence: every sync equals the model", "sequence: a repack that kept the capacity", "sequence: a repack that grew the capacity",
                 "sequence: the headers grew past the initial keyframe capacity"):
        _case(report, name)
    trace = R.parse_trace(ln for ln in report if ln.startswith("trace "))
    assert len(trace) == 40 and trace[-1]["repacks_kept"] >= 1 and trace[-1]["repacks_grown"] >= 2
    assert min(t["n_features"] for t in trace) < trace[0]["n_features"] * 0.5          # most keyframes were culled at once
    assert trace[-1]["n_features"] > trace[11]["n_features"] * 2                       # ... and came back
    assert all(t["pool_used"] <= t["pool_capacity"] and t["n_features"] <= t["pool_used"] for t in trace)


def test_entries_without_a_device_bad_arguments_first():
    import ydorbslam_amd as y
    L = y.lib()
    one = (C.c_int32 * 2)(0, 0)
    st = C.c_uint8(0)
    assert L.ydorb_mapdb_enable_features(None) == -1 and b"null handle" in L.ydorb_last_error()
    assert L.ydorb_mapdb_set_keyframe_features(None, None, 0, None, None, None) == -1 and b"null handle" in L.ydorb_last_error()
    assert L.ydorb_mapdb_export_features(None, None, None, None) == -1 and b"null handle" in L.ydorb_last_error()
    assert L.ydorb_mapdb_feat_stats(None, None) == -1 and b"null handle or stats" in L.ydorb_last_error()
    assert L.ydorb_mapdb_fuse_search(None, None, None, 0, one, None, None, None, None, None, None) == -1 and b"null handle" in L.ydorb_last_error()
    assert L.ydorb_mapdb_fuse_search(None, None, None, 1, one, one, C.byref(st), one, C.byref(st), one, C.byref(st)) == -1


def test_python_mirror_and_header_agree_on_the_layouts():
    from ydorbslam_amd._lib import (YdFrustumView, YdFuseTarget, YdMapDbAttrStats, YdMapDbDescStats, YdMapDbFeatStats, YdMapDbRowStats,
                                    YdMapDbStats)
    hdr = open(os.path.join(ROOT, "include", "ydorb", "c_api.h")).read()
    body = hdr[hdr.index("typedef struct YdMapDbFeatStats {"):hdr.index("} YdMapDbFeatStats;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in re.findall(r"int(?:32|64)_t ([^;]+);", body) for n in decl.split(",")]
    assert names == [n for n, _ in YdMapDbFeatStats._fields_] and C.sizeof(YdMapDbFeatStats) == 56
    body = hdr[hdr.index("typedef struct YdFuseTarget {"):hdr.index("} YdFuseTarget;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"\[\d+\]", "", n).strip() for n in re.findall(r"(?:int32_t|float|YdFrustumView) ([^;]+);", body)]
    assert names == [n for n, _ in YdFuseTarget._fields_] and C.sizeof(YdFuseTarget) == 4 + C.sizeof(YdFrustumView) + 32 + 12
    assert (C.sizeof(YdMapDbStats), C.sizeof(YdMapDbRowStats), C.sizeof(YdMapDbDescStats), C.sizeof(YdMapDbAttrStats)) == (72, 56, 80, 40)   # the older four keep their layouts
    for name, value in list(R.STATUS.items()) + [("skip_observed", 1), ("monocular", 2)] + [("target_" + k, v) for k, v in R.TARGET_STATUS.items()]:
        assert re.search(r"#define YDORB_FUSE_%s +%d\b" % (name.upper(), value), hdr), name


@pytest.fixture(scope="module")
def scene():
    return R.Scene()


def test_restatement_agrees_with_the_numpy_statement_of_pass_one(scene):
    """Every (target, point) of the scene, both flag forms: the restatement's status bytes and the bit patterns of u, v, ur of every
    searched entry equal the numpy statement's; r and the level follow from the distance by the table the device uses."""
    import frustum_support as F
    m = R.scene_map(scene)
    rng = np.random.default_rng(11)
    slots = np.arange(scene.n_points, dtype=np.int32)
    seen = {k: 0 for k in R.STATUS.values()}
    for k in range(scene.n_kf):
        for flags in (R.SKIP_OBSERVED, R.MONOCULAR):
            G = scene.target(k, flags=flags)
            skip = (rng.uniform(size=len(slots)) < 0.05).astype(np.uint8)
            r = R.ref_queries(m, [G], [slots], [skip])[0]
            st, u, v, ur, dist = R.numpy_pass1(m, G, slots, skip)
            assert np.array_equal(r["status"], st)
            ok = st == 0
            q = r["queries"]
            for got, want in ((q["u"], u), (q["v"], v), (q["ur"], ur)):
                assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32))
            with np.errstate(all="ignore"):
                lvl = F.table_levels(m["mx"][slots] / dist, F.level_table())
            assert np.array_equal(q["level"][ok], lvl[ok]) and np.array_equal(q["r"][ok].view(np.uint32), (np.float32(scene.th) * R.SF[lvl[ok]]).view(np.uint32))
            assert (q["flags"][ok] == 1).all() and (q["min_level"][ok] == -1).all() and (q["max_level"][ok] == -1).all()
            assert np.array_equal(r["qdesc"][ok], m["desc"][slots][ok])
            assert not q[~ok].view(np.uint8).any() and not r["qdesc"][~ok].any()        # every other status: a zero query, flags 0
            for s in st:
                seen[int(s)] += 1
    assert all(n > 20 for n in seen.values()), seen


def test_restatement_rejects_nan_and_the_half_open_bounds(scene):
    import frustum_support as F
    m = R.scene_map(scene)
    G = scene.target(0, flags=0)
    ok = np.flatnonzero(R.ref_queries(m, [G], [np.arange(scene.n_points)], [np.zeros(scene.n_points, np.uint8)])[0]["status"] == 0)
    p = int(ok[0])
    for field, value in (("pos", np.nan), ("normal", np.nan), ("mn", np.nan), ("mx", np.nan)):
        mm = {k: v.copy() for k, v in m.items()}
        if mm[field].ndim == 2:
            mm[field][p, 0] = value
        else:
            mm[field][p] = value
        assert R.ref_queries(mm, [G], [[p]], [[0]])[0]["status"][0] == R.STATUS["rejected"], field
    q = R.ref_queries(m, [G], [[p]], [[0]])[0]["queries"][0]
    u, v = float(q["u"]), float(q["v"])
    for bounds, want in (((0.0, u, 0.0, 480.0), "rejected"), ((u, 640.0, 0.0, 480.0), "searched"), ((0.0, 640.0, 0.0, v), "rejected"),
                         ((0.0, 640.0, v, 480.0), "searched")):
        Gb = scene.target(0, flags=0, bounds=bounds)
        assert R.ref_queries(m, [Gb], [[p]], [[0]])[0]["status"][0] == R.STATUS[want], bounds
