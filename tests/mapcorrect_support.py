"""Test support of the map correction on the resident table (ydorb_mapdb_correct): builds the CPU restatement
tests/mapcorrect_ref/mapcorrect_ref.cpp with oracle/Makefile's flags the way mapmaint_support.ref() does, runs it on flat tables through
the product's own argument preparation (ydorbslam_amd.map_resident.correction), and makes the seeded scene, the transforms and the three
call shapes (loops A, B, C of the entry's header comment) the CPU and GPU tests share.  Every comparison is exact."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import mapmaint_support as S
from mapmaint_support import ROOT

SRC = os.path.join(ROOT, "tests", "mapcorrect_ref", "mapcorrect_ref.cpp")
CHECK_SRC = os.path.join(ROOT, "tests", "cpu_harness", "mapdb_correct_check.cpp")
SEED = 5
DONE, BAD, CLAIMED, NOT_COVERED, DONE_NO_OBS = 0, 1, 2, 3, 4
_REF = None


def ref():
    global _REF
    if _REF is None:
        out = os.path.join(tempfile.mkdtemp(prefix="mapcorr"), "libmapcorrref.so")
        subprocess.check_call(["g++", *S._flags(), "-shared", "-o", out, SRC, "-lm"])
        L = C.CDLL(out)
        L.mapcorrect_ref.restype, L.mapcorrect_ref.argtypes = C.c_int, [C.c_void_p] * 6
        _REF = L
    return _REF


def ref_correct(m, kf_slots, before, after, slots=None, corrector=None, arithmetic="sim3", centre_after=None, centres="resident",
                scale_factors=None):
    """The restatement on the flat table m = dict(table, pos, centre, ref_kf, ref_level, ...).  Returns (outputs as MapDb.correct's,
    the table afterwards: a copy of m with the new pos and centre)."""
    from ydorbslam_amd.map_resident import correction
    T = m["table"]
    corr, out, _keep = correction(kf_slots, before, after, T.n_points if slots is None else None, slots, corrector, arithmetic, centre_after,
                                  centres, scale_factors)
    pos, centre = np.array(m["pos"], np.float32, copy=True), np.array(m["centre"], np.float32, copy=True)
    ref_kf, ref_level = np.ascontiguousarray(m["ref_kf"], np.int32), np.ascontiguousarray(m["ref_level"], np.uint8)
    assert ref().mapcorrect_ref(C.byref(T.struct), S._p(pos), S._p(centre), S._p(ref_kf), S._p(ref_level), C.byref(corr)) == 0
    after_m = dict(m)
    after_m.update(pos=pos, centre=centre)
    return out, after_m


def same_correction(got, want):
    """Status bytes and the bit patterns of every float, keys of both sides."""
    assert sorted(got) == sorted(want)
    assert np.array_equal(got["status"], want["status"])
    for k in got:
        if k != "status":
            assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint32), np.ascontiguousarray(want[k]).view(np.uint32)), k


# ------------------------------------------------------------------------------------------------------------ scene and transforms
def scene(seed=SEED, n_keyframes=40, n_points=600):
    """The seeded map of the tests: 0 .. 12 observers per point (some spans empty), 5 % of the points bad."""
    return S.random_map(seed, n_keyframes, n_points, min_obs=0, max_obs=12, bad_share=0.05)


def _quat(rng, n, angle):
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    a = rng.uniform(-angle, angle, (n, 1))
    q = np.concatenate([axis * np.sin(a / 2), np.cos(a / 2)], axis=1)
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def sim3_pairs(seed, n):
    """before / after [n, 8] doubles (qx qy qz qw tx ty tz s): arbitrary poses with scale 1 and a corrected version of each, rotated by
    up to 0.2 rad more, moved by up to 0.5 and scaled by 0.9 .. 1.1.  Inputs only: neither side of a comparison derives them."""
    rng = np.random.default_rng(seed)
    before = np.concatenate([_quat(rng, n, np.pi), rng.uniform(-4, 4, (n, 3)), np.ones((n, 1))], axis=1)
    after = np.concatenate([_quat(rng, n, np.pi), before[:, 4:7] + rng.uniform(-0.5, 0.5, (n, 3)), rng.uniform(0.9, 1.1, (n, 1))], axis=1)
    after[:, :4] = before[:, :4] + rng.uniform(-0.1, 0.1, (n, 4))
    after[:, :4] /= np.linalg.norm(after[:, :4], axis=1, keepdims=True)
    return np.ascontiguousarray(before, np.float64), np.ascontiguousarray(after, np.float64)


def se3_pairs(seed, n):
    """before [n, 12] floats = Rcw | tcw, after [n, 12] = Rwc | twc of a slightly different pose."""
    rng = np.random.default_rng(seed)

    def rot(q):
        x, y, z, w = q
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    qb, dq = _quat(rng, n, np.pi), _quat(rng, n, 0.1)
    before, after = np.zeros((n, 12), np.float32), np.zeros((n, 12), np.float32)
    for i in range(n):
        Rcw, tcw = rot(qb[i]), rng.uniform(-4, 4, 3)
        Rcw2, tcw2 = rot(dq[i]) @ Rcw, tcw + rng.uniform(-0.3, 0.3, 3)
        before[i] = np.concatenate([Rcw.reshape(-1), tcw])
        after[i] = np.concatenate([Rcw2.T.reshape(-1), -Rcw2.T @ tcw2])
    return before, after


def new_centres(seed, m, kf_slots):
    rng = np.random.default_rng(seed)
    return (np.asarray(m["centre"], np.float32)[kf_slots] + rng.uniform(-0.5, 0.5, (len(kf_slots), 3))).astype(np.float32)


def shape_a(m, seed=1, window=14):
    """Loop A: `window` keyframes in a shuffled order, the entries = their map-point lists concatenated, corrector = the list's rank;
    the third keyframe lists its first point twice.  Each list lacks a seeded 30 % of the points that record the keyframe as an observer
    (a map-point vector and the observation maps disagree after a fuse or a replace): with complete lists the first observer in the order
    always claims, no point would have an observer before its corrector, and the interleaved rule would show nothing.  Returns the
    keyword arguments of MapDb.correct / ref_correct."""
    rng = np.random.default_rng(seed)
    kf = rng.permutation(m["table"].n_keyframes)[:window].astype(np.int32)
    lists = [[p for p in m["kf_points"][k] if rng.uniform() >= 0.3] for k in kf]
    if lists[2]:
        lists[2].append(lists[2][0])
    slots = np.concatenate([np.asarray(a, np.int32) for a in lists])
    corrector = np.concatenate([np.full(len(a), r, np.int32) for r, a in enumerate(lists)])
    before, after = sim3_pairs(seed + 100, window)
    return dict(kf_slots=kf, before=before, after=after, slots=slots, corrector=corrector, arithmetic="sim3", centre_after=new_centres(seed + 200, m, kf),
                centres="interleaved", scale_factors=S.scale_factors())


def shape_b(m, seed=2, claimed_by_a=None):
    """Loop B: every keyframe, slots None, corrector = a rank for the points loop A claimed (here: a seeded third of them), -1 elsewhere."""
    rng = np.random.default_rng(seed)
    T = m["table"]
    kf = rng.permutation(T.n_keyframes).astype(np.int32)
    corrector = np.full(T.n_points, -1, np.int32)
    pick = rng.uniform(size=T.n_points) < 0.33 if claimed_by_a is None else claimed_by_a
    corrector[pick] = rng.integers(0, T.n_keyframes, int(pick.sum()))
    before, after = sim3_pairs(seed + 100, T.n_keyframes)
    return dict(kf_slots=kf, before=before, after=after, slots=None, corrector=corrector, arithmetic="sim3", centre_after=new_centres(seed + 200, m, kf),
                centres="poses_first", scale_factors=S.scale_factors())


def shape_c(m, seed=3, reached=30):
    """Loop C: SE3, no normals, -1 correctors, only the reached keyframes in kf_slots: the other points come back NOT_COVERED."""
    rng = np.random.default_rng(seed)
    kf = rng.permutation(m["table"].n_keyframes)[:reached].astype(np.int32)
    before, after = se3_pairs(seed + 100, reached)
    return dict(kf_slots=kf, before=before, after=after, slots=None, corrector=None, arithmetic="se3", centre_after=None, centres="resident",
                scale_factors=None)


SHAPES = dict(A=shape_a, B=shape_b, C=shape_c)


def with_entries(args, n):
    """The first n entries of a call (slots None: the slots 0 .. n-1 by name)."""
    a = dict(args)
    a["slots"] = np.arange(n, dtype=np.int32) if args["slots"] is None else args["slots"][:n]
    a["corrector"] = None if args["corrector"] is None else args["corrector"][:n]
    return a


def build_run_exe(out):
    lib_dir = os.path.join(ROOT, "ydorbslam_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpu_harness", "mockrt"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp_host", "mapcorrect_run.cpp"), "-o", out,
                           "-L" + lib_dir, "-l:libydorb.so", "-Wl,-rpath," + lib_dir])
    return out


def run_adapter(exe, tmp, adapter_scene, current, covisible):
    """Runs tests/cpp_host/mapcorrect_run.cpp on a mapmaint_support.adapter_scene.  Returns {name: int}."""
    inp = os.path.join(tmp, "in.bin")
    open(inp, "wb").write(S.adapter_blob(adapter_scene, current, covisible, [], S.scale_factors()))
    r = subprocess.run([exe, inp], stdout=subprocess.PIPE, text=True, check=True)
    return {ln.split()[0]: int(ln.split()[1]) for ln in r.stdout.splitlines()}


def build_check_exe(out, sanitize):
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, CHECK_SRC, "-o", out])
    return out
