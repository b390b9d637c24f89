"""The map correction on the resident table without a GPU: the CPU restatement (tests/mapcorrect_ref/mapcorrect_ref.cpp) on
hand-computed cases, the proof that the seeded scene of the GPU tests can tell the interleaved order from poses-first, the sanitized
stand-alone check of the host planning in ydorbslam_amd/csrc/mapdb_host.h (tests/cpu_harness/mapdb_correct_check.cpp, its own process:
nothing is loaded into this one under a sanitizer), what the entry does on a machine with no device, and the adapter's type check."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mapcorrect_support as K
import mapmaint_support as S
from mapmaint_support import ROOT

f32 = np.float32
IDENTITY = np.array([[0, 0, 0, 1, 0, 0, 0, 1]], np.float64)


def _one_kf_map(points):
    """One keyframe at the origin observing every point once."""
    from ydorbslam_amd.map_maintenance import ObservationTable
    n = len(points)
    T = ObservationTable(1, [np.zeros(1, np.int32)] * n, [np.zeros(1, np.uint8)] * n, [np.zeros(1, np.uint8)] * n, np.zeros(n, np.uint8))
    return dict(table=T, pos=np.array(points, f32), centre=np.zeros((1, 3), f32), ref_kf=np.zeros(n, np.int32), ref_level=np.zeros(n, np.uint8))


POINTS = [[1.5, -2.25, 3.0], [0.1, 0.2, 0.3], [-7.0, 11.0, 13.0]]


# ------------------------------------------------------------------------------------------------------------ (a) hand-computed
def test_identity_pair_returns_the_positions_bit_for_bit():
    m = _one_kf_map(POINTS)
    out, after = K.ref_correct(m, [0], IDENTITY, IDENTITY)
    assert np.array_equal(out["status"], [K.DONE] * 3)
    assert np.array_equal(out["pos"].view(np.uint32), m["pos"].view(np.uint32)) and np.array_equal(after["pos"].view(np.uint32), m["pos"].view(np.uint32))
    eye = np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]], f32)
    out, _ = K.ref_correct(m, [0], eye, eye, arithmetic="se3")
    assert np.array_equal(out["pos"].view(np.uint32), m["pos"].view(np.uint32))


def test_pure_scale():
    """after = the identity with scale 1/2: correctedSwi scales by 2, exactly; the distances follow the new position."""
    m = _one_kf_map(POINTS)
    half = IDENTITY.copy()
    half[0, 7] = 0.5
    sf = S.scale_factors(1.5, 2)
    out, after = K.ref_correct(m, [0], IDENTITY, half, scale_factors=sf)
    want = m["pos"] * f32(2)
    assert np.array_equal(out["pos"].view(np.uint32), want.view(np.uint32)) and np.array_equal(after["pos"], want)
    w = want.astype(np.float64)
    norm = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
    dist = norm.astype(f32)
    assert np.array_equal(out["max_distance"], dist) and np.array_equal(out["min_distance"], dist / f32(1.5))
    unit = want * (1.0 / norm).astype(f32)[:, None]                 # one observer: the normal is the point scaled by float(1 / norm)
    assert unit.dtype == f32 and np.array_equal(out["normal"], unit)


def test_quarter_turn():
    """SE3: Rcw = a quarter turn about z, tcw = (1, 2, 3), the inverse pose after = the identity: P' = Rz P + t, exact in small integers.
    Sim3: the same turn as a quaternion (sqrt(1/2) is not exact in double, the float result is)."""
    pts = [[1, 2, 3], [-4, 5, 6], [8, -16, 32]]
    m = _one_kf_map(pts)
    before = np.array([[0, -1, 0, 1, 0, 0, 0, 0, 1, 1, 2, 3]], f32)
    eye = np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]], f32)
    out, _ = K.ref_correct(m, [0], before, eye, arithmetic="se3")
    want = np.array([[-2 + 1, 1 + 2, 3 + 3], [-5 + 1, -4 + 2, 6 + 3], [16 + 1, 8 + 2, 32 + 3]], f32)
    assert np.array_equal(out["pos"], want)
    h = np.sqrt(0.5)
    turn = np.array([[0, 0, h, h, 0, 0, 0, 1]], np.float64)
    out, _ = K.ref_correct(m, [0], turn, IDENTITY)
    assert np.array_equal(out["pos"], np.array([[-2, 1, 3], [-5, -4, 6], [16, 8, 32]], f32))
    out, _ = K.ref_correct(m, [0], IDENTITY, turn)                  # the entry inverts `after`: a quarter turn back
    assert np.array_equal(out["pos"], np.array([[2, -1, 3], [5, 4, 6], [-16, -8, 32]], f32))


def test_status_and_centres_on_a_small_table():
    """bad, claimed, not covered and the empty span, and the centre array afterwards."""
    from ydorbslam_amd.map_maintenance import ObservationTable
    obs = [[0, 1], [1], [], [2]]
    T = ObservationTable(3, [np.array(o, np.int32) for o in obs], [np.zeros(len(o), np.uint8) for o in obs], [np.zeros(len(o), np.uint8) for o in obs],
                         np.array([0, 1, 0, 0], np.uint8))
    m = dict(table=T, pos=np.arange(12, dtype=f32).reshape(4, 3) + 1, centre=np.zeros((3, 3), f32), ref_kf=np.array([0, 1, 1, 2], np.int32),
             ref_level=np.zeros(4, np.uint8))
    two = np.repeat(IDENTITY, 2, axis=0)
    cen = np.array([[9, 9, 9], [7, 7, 7]], f32)
    out, after = K.ref_correct(m, [1, 0], two, two, slots=[1, 0, 0, 2, 3], corrector=[0, 1, 0, -1, -1], centre_after=cen, centres="interleaved",
                               scale_factors=S.scale_factors())
    assert np.array_equal(out["status"], [K.BAD, K.DONE, K.CLAIMED, K.DONE_NO_OBS, K.NOT_COVERED])
    assert np.array_equal(out["pos"], [[0, 0, 0], [1, 2, 3], [0, 0, 0], [7, 8, 9], [0, 0, 0]])
    assert np.array_equal(after["centre"], [[7, 7, 7], [9, 9, 9], [0, 0, 0]])
    assert not out["normal"][[0, 2, 3, 4]].any() and out["normal"][1].any()


# ------------------------------------------------------------------------------------------------------------ (b) the order is visible
def test_the_seeded_scene_tells_interleaved_from_poses_first():
    m = K.scene()
    a = K.shape_a(m)
    inter, _ = K.ref_correct(m, **a)
    first, _ = K.ref_correct(m, **dict(a, centres="poses_first"))
    assert np.array_equal(inter["status"], first["status"]) and np.array_equal(inter["pos"].view(np.uint32), first["pos"].view(np.uint32))
    differs = (inter["normal"].view(np.uint32) != first["normal"].view(np.uint32)).any(axis=1)
    assert differs.any()
    rank_of = {int(k): r for r, k in enumerate(a["kf_slots"])}
    both_sides = 0
    for i in np.flatnonzero(inter["status"] == K.DONE):
        r = int(a["corrector"][i])
        ranks = [rank_of[int(k)] for k in m["observers"][a["slots"][i]] if int(k) in rank_of]
        both_sides += any(x < r for x in ranks) and any(x > r for x in ranks)
    assert both_sides >= 1
    st = inter["status"]
    assert all((st == code).any() for code in (K.DONE, K.BAD, K.CLAIMED))             # the scene meets these by itself
    b, _ = K.ref_correct(m, **K.shape_b(m))
    c, _ = K.ref_correct(m, **K.shape_c(m))
    assert (b["status"] == K.DONE_NO_OBS).any() and (c["status"] == K.NOT_COVERED).any() and (c["status"] == K.DONE).any()


# ------------------------------------------------------------------------------------------------------------ (c) the sanitized program
@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = K.build_check_exe(str(tmp_path_factory.mktemp("mapcorr") / "mapdb_correct_check"), sanitize=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    return r.stdout.splitlines()


def _case(report, name):
    hits = [ln for ln in report if ln.startswith(name + " ")]
    assert len(hits) == 1 and " ok" in hits[0] and "FAILED" not in hits[0], (name, hits)
    return hits[0]


def test_correct_check_runs_clean_under_the_sanitizers(report):
    assert report[-1] == "0 failed" and len(report) == 36 and not any("FAILED" in ln for ln in report)


def test_every_validation_message_of_the_correction(report):
    for name in ("null correction", "unknown arithmetic", "unknown centres", "negative n_kf", "negative n", "centres without centre_after", "null kf_slots",
                 "null after", "null status", "two of three normal outputs", "n_levels 9", "n_levels 0", "null scale_factors", "null slots, n != n_points",
                 "keyframe slot out of range", "keyframe slot negative", "keyframe slot repeated", "Sim3 scale zero", "Sim3 scale negative",
                 "Sim3 scale NaN", "Sim3 scale infinite", "point slot out of range", "point slot negative", "corrector out of range", "corrector below -1",
                 "ref_level >= n_levels of a corrected point", "no normals: the level is not read", "a refused call changes neither mirror nor staging"):
        _case(report, name)


def test_the_claim_pass_and_the_mirror(report):
    for name in ("well formed", "claim: the first entry that is not bad claims", "claim: named 3 times, the first bad, the second claims",
                 "claim: -1 correctors, covered and not covered", "claim: null slots", "the mirror after applying a result",
                 "n == 0 with centres; no keyframes"):
        _case(report, name)


# ------------------------------------------------------------------------------------------------------------ (d) no device, the adapter
def test_correct_without_a_device_is_no_device():
    import ydorbslam_amd as y
    from ydorbslam_amd._lib import YdMapCorrection
    L = y.lib()
    c = YdMapCorrection()
    rc = L.ydorb_mapdb_correct(None, C.byref(c))
    if L.ydorb_device_count() == 0:
        assert rc == -2                                                        # YDORB_ERR_NO_DEVICE: there is no CPU fallback
    else:
        assert rc == -1 and b"null handle" in L.ydorb_last_error()


def test_python_mirror_and_header_agree_on_the_correction_layout():
    import re
    from ydorbslam_amd._lib import YdMapCorrection
    hdr = open(os.path.join(ROOT, "include", "ydorb", "c_api.h")).read()
    body = re.sub(r"/\*.*?\*/", "", hdr[hdr.index("typedef struct YdMapCorrection {"):hdr.index("} YdMapCorrection;")], flags=re.S)
    names = [n.strip(" *") for decl in re.findall(r"(?:const )?(?:int32_t|void|float|uint8_t)\*? ([^;]+);", body) for n in decl.split(",")]
    assert names == [n for n, _ in YdMapCorrection._fields_] and C.sizeof(YdMapCorrection) == 120
    for name, value in (("SIM3", 0), ("SE3", 1), ("RESIDENT", 0), ("INTERLEAVED", 1), ("POSES_FIRST", 2), ("DONE", 0), ("BAD", 1), ("CLAIMED", 2),
                        ("NOT_COVERED", 3), ("DONE_NO_OBSERVATIONS", 4)):
        assert re.search(r"#define YDORB_MAPCORR_%s %d\b" % (name, value), hdr), name


def test_map_correction_adapter_typechecks():
    """The three correction methods of include/ydorb/mapMirror.hpp against declarations of the members they use."""
    H = os.path.join(ROOT, "tests", "cpu_harness")
    subprocess.check_call(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-I" + os.path.join(H, "mock"), os.path.join(H, "mapcorrect_syntax_check.cpp")])
