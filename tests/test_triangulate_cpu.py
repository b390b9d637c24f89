"""createNewMapPoints' geometry without a GPU: the CPU restatement (tests/triangulate_ref) against ground truth, numpy and hand-built
cases, the adapter's syntax check and the ABI's argument checks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import triangulate_support as S
from triangulate_support import ROOT


def _noise_free_scenes():
    """Known points seen by two keyframes without pixel noise, for each source: (views, problem, truth [n, 3], wanted status)."""
    rng = np.random.default_rng(3)
    n = 60
    z = rng.uniform(2.0, 10.0, n)
    X = np.stack([rng.uniform(-0.45, 0.45, n) * z, rng.uniform(-0.35, 0.35, n) * z, z], axis=1)   # inside both images, right_x >= 0
    out = []
    for src, centre in ((1, (0.45, 0.03, 0.05)), (2, (0.02, 0.0, 0.0)), (3, (0.02, 0.0, 0.0))):
        T = [S.pose(), S.pose(S.rot((0.1, 1, 0.05), np.radians(2.0 if src == 1 else 0.0)), centre)]
        vb = [S.ViewBuilder(t) for t in T]
        for k in range(n):
            for v in range(2):
                uv, z = S.project(T[v], X[k:k + 1])
                vb[v].add(uv[0], 0, z[0] if (src == 2 and v == 0) or (src == 3 and v == 1) else None)
        idx = np.arange(n, dtype=np.int32)
        out.append(([v.view() for v in vb], dict(first=0, second=1, idx1=idx, idx2=idx), X, src << 4))
    return out


def _numpy_solution(views, prob, src):
    """The same float inputs solved in double: numpy SVD of A for the linear source, the unprojection formula for the stereo ones."""
    f64 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    V1, V2 = views[prob["first"]], views[prob["second"]]
    pts = []
    for i1, i2 in zip(prob["idx1"], prob["idx2"]):
        if src == 1:
            rows = []
            for V, i in ((V1, i1), (V2, i2)):
                T = f64(V["Tcw"])
                xn = (f64(V["kps"]["x"][i]) - f64(V["cx"])) * f64(V["invfx"]), (f64(V["kps"]["y"][i]) - f64(V["cy"])) * f64(V["invfy"])
                rows += [xn[0] * T[2] - T[0], xn[1] * T[2] - T[1]]
            h = np.linalg.svd(np.array(rows))[2][3]
            pts.append(h[:3] / h[3])
        else:
            V, i = (V1, i1) if src == 2 else (V2, i2)
            z = f64(V["depth"][i])
            xc = np.array([(f64(V["kps"]["x"][i]) - f64(V["cx"])) * z * f64(V["invfx"]), (f64(V["kps"]["y"][i]) - f64(V["cy"])) * z * f64(V["invfy"]), z])
            pts.append(f64(V["Rwc"]) @ xc + f64(V["Ow"]))
    return np.array(pts)


FP32_MARGIN = 64.0


def test_noise_free_points_are_recovered():
    """Every noise-free match is accepted from the expected source and the point is the true one.  Tolerance, per source: the largest
    error of the double-precision solution of the SAME float inputs (so: the effect of rounding the ~16 inputs to float once each)
    times FP32_MARGIN = 64.  Reasoning for the margin, fixed before the first run: the float path rounds about 750 times (8 entries
    of A, then ~5 sweeps of 6 rotations over 8 elements at 3 roundings each, then the division), each rounding the size of one input
    rounding and amplified by the same conditioning; as a random walk that is sqrt(750 / 16) ~ 7 times the double solution's error,
    in the worst case 750 / 16 ~ 47 times.  Measured (printed below; DESIGN.md section 6f records them)."""
    for views, prob, truth, want in _noise_free_scenes():
        r = S.ref_triangulate(views, [prob])[0]
        assert np.all(r["status"] == want), (want, np.unique(r["status"]))
        err64 = np.abs(_numpy_solution(views, prob, want >> 4) - truth).max()
        err32 = np.abs(r["x3d"].astype(np.float64) - truth).max()
        print("source %d: double solution of the float inputs %.3e m, restatement %.3e m, ratio %.1f" % (want >> 4, err64, err32, err32 / err64))
        assert err32 <= FP32_MARGIN * err64


GAP_FLOOR = 0.02


def test_jacobi_null_vector_matches_numpy_svd():
    """The right singular vector of the smallest singular value against numpy.linalg.svd in double, on random float 4x4 matrices whose
    relative gap (s3 - s4) / s1 is at least GAP_FLOOR = 0.02: below it the vector is ill-conditioned in any fp32 solver.  The floor
    leaves out at most 10 % of the draws (checked).  A singular vector's error is bounded by (error of A) / gap: A's float entries
    carry 2^-24 relative to s1 and the Jacobi accumulates some tens of roundings, so 64 * 2^-24 / GAP_FLOOR = 1.9e-4."""
    rng = np.random.default_rng(11)
    n, kept, worst, sweeps = 2000, 0, 0.0, 0
    for _ in range(n):
        A = rng.normal(size=(4, 4)).astype(np.float32)
        s, vt = np.linalg.svd(A.astype(np.float64))[1:]
        if (s[2] - s[3]) / s[0] < GAP_FLOOR:
            continue
        kept += 1
        x, it = S.ref_null_vector(A)
        sweeps = max(sweeps, it)
        x = x.astype(np.float64)
        assert abs(np.linalg.norm(x) - 1) < 1e-5
        worst = max(worst, min(np.abs(x - vt[3]).max(), np.abs(x + vt[3]).max()))
    print("kept %d of %d, worst component error %.3e, most sweeps %d" % (kept, n, worst, sweeps))
    assert kept >= 0.9 * n
    assert worst <= 64 * 2.0 ** -24 / GAP_FLOOR
    assert sweeps < 30            # the bound is a guard, not the stopping rule


def test_null_vector_sign_invariance_and_nan_termination():
    rng = np.random.default_rng(5)
    A = rng.normal(size=(4, 4)).astype(np.float32)
    x, _ = S.ref_null_vector(A)
    y, _ = S.ref_null_vector(-A)
    assert np.array_equal((x[:3] / x[3]).view(np.uint32), (y[:3] / y[3]).view(np.uint32))
    A[1, 2] = np.nan
    x, it = S.ref_null_vector(A)
    assert it == 30 and np.isnan(x).any()


def _ulps(a, b):
    """Distance between float32 values in units in the last place (monotone integer mapping of the bit patterns)."""
    def key(x):
        i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def test_rational_stereo_parallax_against_libm():
    """(d^2 - h^2) / (d^2 + h^2), h = b / 2, against the reference's float chain cosf(2 * atan2f(b / 2, d)) of the C library, over
    3000 log-spaced depths in 0.1-100 m, for the baselines 0.08, 0.12 (h below the range: the cosine stays near 1) and 0.54 m (KITTI;
    the cosine crosses 0 at d = h inside the range).  Measured with glibc's libm: the two forms differ by at most 2 units of 2^-24
    (2 float ulp of 1) at every baseline, which is at most 3 ulp of the value itself for the two short baselines; near the zero
    crossing of the long one the same absolute gap is hundreds of ulp of the (tiny) value, 594 at the worst depth, which is the libm
    chain's cancellation, not ours: against cos(2 atan2) evaluated in double and rounded, the rational form is 0 ulp off everywhere.
    Asserted at the measured values times 1.5, rounded up: 3 units of 2^-24, 4 ulp of the value for the short baselines and 891 for
    the long one; 1 ulp against the double evaluation (one final rounding of a double that carries three roundings of its own)."""
    libm = C.CDLL("libm.so.6")
    libm.cosf.restype = libm.atan2f.restype = C.c_float
    libm.cosf.argtypes, libm.atan2f.argtypes = [C.c_float], [C.c_float, C.c_float]
    d = np.exp(np.linspace(np.log(0.1), np.log(100.0), 3000)).astype(np.float32)
    for b in (0.08, 0.12, 0.54):
        h = np.float32(b) / np.float32(2)
        ours = np.array([S.ref_cos_stereo(b, float(x)) for x in d], np.float32)
        chain = np.array([libm.cosf(np.float32(2) * np.float32(libm.atan2f(h, x))) for x in d], np.float32)
        exact = np.cos(2 * np.arctan2(np.float64(h), d.astype(np.float64))).astype(np.float32)
        gap_abs = np.abs(ours.astype(np.float64) - chain.astype(np.float64)).max() * 2.0 ** 24
        gap_ulp, gap_exact = int(_ulps(ours, chain).max()), int(_ulps(ours, exact).max())
        print("b = %.2f: vs libm chain %.1f units of 2^-24, %d ulp of the value; vs double evaluation %d ulp" % (b, gap_abs, gap_ulp, gap_exact))
        assert gap_abs <= 3
        assert gap_exact <= 1
        assert gap_ulp <= (4 if b < 0.2 else 891)


@pytest.mark.parametrize("name", sorted(S.hand_cases()))
def test_hand_built_case_gives_its_exit_code(name):
    views, prob, want = S.hand_cases()[name]
    r = S.ref_triangulate(views, [prob])[0]
    assert r["status"][0] == want, (name, hex(r["status"][0]), hex(want))
    assert r["n_accepted"] == int((want & 15) == 0)
    finite = np.isfinite(r["x3d"][0]).all()
    assert bool(want & 0x80) == (not finite)
    if (want & 15) in (1, 2, 9):
        assert not r["x3d"][0].any()


def test_hand_built_cases_cover_every_exit_and_source():
    want = [st for _, _, st in S.hand_cases().values()]
    assert {s & 15 for s in want} == set(range(10))
    assert {(s >> 4) & 3 for s in want} == {0, 1, 2, 3}
    assert 0xA0 in want            # the NaN point the reference accepts


def test_scene_takes_every_branch():
    """The GPU tests' scene, on the restatement: every exit 0-8 and every source occurs."""
    views, problems = S.scene()
    st = np.concatenate([r["status"] for r in S.ref_triangulate(views, problems)])
    assert set((st & 15).tolist()) >= set(range(9))
    assert set(((st >> 4) & 3).tolist()) == {0, 1, 2, 3}


def test_local_mapping_adapter_typechecks():
    H = os.path.join(ROOT, "tests", "cpu_harness")
    subprocess.check_call(["g++", "-std=c++14", "-fsyntax-only", "-I" + os.path.join(H, "mock"), os.path.join(H, "localmapping_syntax_check.cpp")])


def test_abi_rejects_bad_arguments_without_a_gpu():
    """Index and shape errors are reported before any device work, so this runs anywhere."""
    import ydorbslam_amd as y
    from ydorbslam_amd.triangulate import TriBatch, triangulate_matches
    y.build_library()
    views, prob, _ = S.hand_cases()["accepted_linear"]
    L = y.lib()

    def rejected(views, problems, match):
        with pytest.raises(y.YdorbError, match=match):
            triangulate_matches(views, problems)

    rejected(views, [dict(prob, second=2)], "view index out of range")
    rejected(views, [dict(prob, first=-1)], "view index out of range")
    rejected(views, [dict(prob, idx1=[1])], "keypoint index")
    rejected(views, [dict(prob, idx2=[-1])], "keypoint index")
    bad = [dict(views[0]), views[1]]
    bad[0]["kps"] = views[0]["kps"].copy()
    bad[0]["kps"]["octave"][0] = 8
    rejected(bad, [prob], "octave")
    B = TriBatch(views, [prob])
    x3d, status, nacc = B.outputs()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.ydorb_triangulate_matches(None, p(x3d), p(status), p(nacc)) == -1
    assert L.ydorb_triangulate_matches(C.byref(B.struct), None, p(status), p(nacc)) == -1
    B.start[1] = -1
    assert L.ydorb_triangulate_matches(C.byref(B.struct), p(x3d), p(status), p(nacc)) == -1
    assert b"match_start" in L.ydorb_last_error()
    B.start[1] = 1
    B.struct.device = 16
    assert L.ydorb_triangulate_matches(C.byref(B.struct), p(x3d), p(status), p(nacc)) == -1
    assert L.ydorb_triangulate_release(-1) == -1
