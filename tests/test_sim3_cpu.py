"""The loop-closure Sim3 check without a GPU: the CPU restatement's known answers (tests/sim3_ref), setRansacParameters, the fp32
contract's quaternion-to-R against the reference's atan2 -> Rodrigues, the ABI's symbols and layouts, and the fail-loud path."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from sim3_support import ROOT, ref, ref_horn, ref_ransac, rot, synth_ransac


def umeyama(X1, X2, fix_scale):
    """X1 ~ s R X2 + t by SVD (Umeyama 1991)."""
    m1, m2 = X1.mean(0), X2.mean(0)
    A, B = X1 - m1, X2 - m2
    U, D, Vt = np.linalg.svd(A.T @ B)
    S = np.diag([1, 1, np.sign(np.linalg.det(U @ Vt))])
    R = U @ S @ Vt
    s = 1.0 if fix_scale else np.trace(np.diag(D) @ S) / (B ** 2).sum()
    return R, m1 - s * R @ m2, s


def horn_gap(X1, X2):
    """Relative gap between the two largest eigenvalues of Horn's 4x4 (fp64).  Three points are coplanar, so the spectrum comes in
    near +- pairs; a small gap makes the leading eigenvector ill-conditioned in any fp32 eigen solver, the reference's cv::eigen too."""
    P1, P2 = X1.T - X1.T.mean(1, keepdims=True), X2.T - X2.T.mean(1, keepdims=True)
    M = P2 @ P1.T
    N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                  [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                  [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]], [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]])
    w = np.linalg.eigvalsh(np.triu(N) + np.triu(N, 1).T)
    return (w[3] - w[2]) / abs(w).max()


@pytest.mark.parametrize("fix_scale", [True, False])
def test_horn_recovers_a_noise_free_sim3(fix_scale):
    rng = np.random.default_rng(3)
    checked = 0
    for trial in range(40):
        R = rot(rng, 2.5)
        t = rng.uniform(-2, 2, 3)
        s = 1.0 if fix_scale else rng.uniform(0.5, 2.0)
        X2 = rng.uniform(-3, 3, (3, 3)) + [0, 0, 6]
        X1 = s * X2 @ R.T + t
        X1f, X2f = X1.astype(np.float32), X2.astype(np.float32)
        if horn_gap(X1f.astype(np.float64), X2f.astype(np.float64)) < 0.05:
            continue
        checked += 1
        h = ref_horn(X1f, X2f, [0, 1, 2], fix_scale)
        assert np.allclose(h["R"], R, rtol=0, atol=1e-5), trial
        assert abs(h["s"] - s) <= 1e-5 * s
        assert np.allclose(h["t"], t, rtol=0, atol=1e-5 * np.abs(X1).max())   # t = O1 - s R O2: relative to the scene
        Ru, tu, su = umeyama(X1f.astype(np.float64), X2f.astype(np.float64), fix_scale)
        assert np.allclose(h["R"], Ru, atol=1e-5) and abs(h["s"] - su) <= 1e-5 * su and np.allclose(h["t"], tu, atol=1e-4)
        if fix_scale:
            assert h["s"] == np.float32(1)
        # T21 inverts T12
        A12, A21 = h["T12"][:9].reshape(3, 3), h["T21"][:9].reshape(3, 3)
        assert np.allclose(A21 @ A12, np.eye(3), atol=1e-5)
    assert checked >= 20


def test_horn_agrees_with_umeyama_on_noisy_triples():
    rng = np.random.default_rng(5)
    for _ in range(50):
        X2 = rng.uniform(-3, 3, (3, 3)) + [0, 0, 6]
        X1 = 1.3 * X2 @ rot(rng, 1.0).T + rng.uniform(-1, 1, 3) + rng.normal(0, 0.01, (3, 3))
        if horn_gap(X1, X2) < 0.05:
            continue
        h = ref_horn(X1.astype(np.float32), X2.astype(np.float32), [0, 1, 2], False)
        Ru, tu, su = umeyama(X1.astype(np.float32).astype(np.float64), X2.astype(np.float32).astype(np.float64), False)
        assert np.allclose(h["R"], Ru, atol=2e-5) and abs(h["s"] - su) <= 2e-5 * su


def test_ransac_iteration_count():
    from ydorbslam_amd.sim3 import ransac_iterations
    L = ref()
    assert ransac_iterations(20, 0.99, 20, 300) == 1 == L.sim3ref_ransac_its(20, 0.99, 20, 300)   # minInliers == N
    for N in (21, 25, 30, 50, 100, 300, 2000):
        it = ransac_iterations(N, 0.99, 20, 300)
        assert it == L.sim3ref_ransac_its(N, 0.99, 20, 300), N
        eps = np.float32(20) / np.float32(N)
        assert it == max(1, min(300, int(np.ceil(np.log(0.01) / np.log(1 - float(eps) ** 3)))))
    assert ransac_iterations(50, 0.99, 20, 300) == 70
    assert ransac_iterations(21, 0.99, 20, 300) == 3
    assert ransac_iterations(10, 0.99, 20, 300) == 1 == L.sim3ref_ransac_its(10, 0.99, 20, 300)   # minInliers > N: NaN count


def test_quaternion_rotation_matches_atan2_rodrigues():
    """The contract builds R from the normalised quaternion; the reference takes ang = atan2(|v|, w) and Rodrigues(2 ang v / |v|).
    Equal in exact arithmetic; in float the two differ by a few ulp."""
    rng = np.random.default_rng(11)
    worst = 0
    for _ in range(2000):
        q = rng.normal(size=4).astype(np.float32)
        q /= np.float32(np.linalg.norm(q))
        q = q.astype(np.float32)
        if q[0] < 0:
            q = -q
        w, x, y, z = (np.float32(v) for v in q)
        n = np.sqrt(np.float32(((w * w + x * x) + y * y) + z * z))
        w, x, y, z = w / n, x / n, y / n, z / n
        one, two = np.float32(1), np.float32(2)
        Rq = np.array([one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y), two * (x * y + w * z), one - two * (x * x + z * z),
                       two * (y * z - w * x), two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)], np.float32)
        Rr = np.zeros(9, np.float32)
        ref().sim3ref_rodrigues(q.ctypes.data_as(C.c_void_p), Rr.ctypes.data_as(C.c_void_p))
        # gap in units of the float ulp at 1 (entries of a rotation lie in [-1, 1])
        worst = max(worst, float(np.abs(Rq.astype(np.float64) - Rr.astype(np.float64)).max() / np.spacing(np.float32(1))))
    print("max gap quaternion vs atan2->Rodrigues: %.1f ulp(1)" % worst)
    assert worst <= 16


def test_oracle_iterate_semantics():
    # N < minInliers: bNoMore at once, nothing evaluated
    p, _ = synth_ransac(19, 1, min_inliers=20, n_hyp=10)
    r = ref_ransac(p, 5)
    assert r["no_more"] and r["ret_hyp"] == -1 and r["next_hyp"] == 0 and r["n_calls"] == 1
    # a clean problem returns at the first hypothesis over minInliers; resuming in pieces reproduces one run
    p, _ = synth_ransac(200, 2, outliers=0.6, min_inliers=20, max_its=40)
    whole = ref_ransac(p, 5)
    assert whole["ret_hyp"] >= 0 and whole["inliers"].sum() == whole["hyp_inliers"][whole["ret_hyp"]] > 20
    st = dict(p, next_hyp=0)
    while True:
        st["triples"] = p["triples"][st["next_hyp"]:st["next_hyp"] + 5]
        r = ref_ransac(st, 5)
        st.update(next_hyp=r["next_hyp"], best_inliers=r["best_inliers"], best_T12=r["best_T12"])
        if r["ret_hyp"] >= 0 or r["no_more"]:
            break
    assert r["ret_hyp"] == whole["ret_hyp"] and np.array_equal(r["inliers"], whole["inliers"])
    assert np.array_equal(r["best_T12"].view(np.uint32), whole["best_T12"].view(np.uint32))


def _header_sizes():
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"ydorb/c_api.h\"\nint main(void){printf(\"%zu %zu %zu %zu\\n\", sizeof(YdSim3Problem), " \
          "sizeof(YdSim3Batch), offsetof(YdSim3Problem, inliers), offsetof(YdSim3Batch, th2));return 0;}\n"
    import tempfile
    d = tempfile.mkdtemp()
    open(os.path.join(d, "s.c"), "w").write(src)
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
    return [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).split()]


def test_sim3_symbols_and_struct_layouts():
    import ydorbslam_amd as y
    from ydorbslam_amd._lib import SYMBOLS, YdSim3Batch, YdSim3Problem
    y.build_library()
    L = C.CDLL(y.library_path())
    for n in ("ydorb_sim3_ransac", "ydorb_sim3_optimize", "ydorb_sim3_release"):
        assert n in SYMBOLS and hasattr(L, n)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ydorb", "c_api.h")).read(), flags=re.S)
    assert "ydorb_sim3_ransac(" in hdr and "ydorb_sim3_optimize(" in hdr
    assert _header_sizes() == [C.sizeof(YdSim3Problem), C.sizeof(YdSim3Batch), YdSim3Problem.inliers.offset, YdSim3Batch.th2.offset]
    assert y.Sim3Solver is y.sim3.Sim3Solver and y.optimize_sim3 is y.sim3.optimize_sim3


def test_sim3_no_cpu_fallback_without_device():
    import torch
    import ydorbslam_amd as y
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the fail-loud path is exercised on CPU-only machines")
    from sim3_support import synth_optimize
    p, _ = synth_ransac(30, 1, n_hyp=5)
    with pytest.raises(y.YdorbError, match="no CPU fallback"):
        y.sim3.ransac([p])
    with pytest.raises(y.YdorbError, match="no CPU fallback"):
        y.optimize_sim3([synth_optimize(20, 1)])
    with pytest.raises(y.YdorbError, match="no CPU fallback"):
        y.sim3.release(0)


def test_sim3_adapters_typecheck():
    """include/ydorb/sim3Solver.hpp and optimizeSim3Impl against declarations of the KeyFrame / MapPoint members they use."""
    h = os.path.join(ROOT, "tests", "cpu_harness")
    subprocess.check_call(["g++", "-std=c++14", "-fsyntax-only", "-I" + os.path.join(h, "mock"), "-I" + os.path.join(h, "mockrt"),
                           os.path.join(h, "sim3_syntax_check.cpp")])


def test_sim3_exp_is_the_matrix_exponential():
    """g2o's Sim3(update) in closed form (A, B, C branches of sim3.h, restated by the oracle and the kernel) against an independent
    matrix exponential of the sim(3) generator [[Omega + sigma I, upsilon], [0, 0]]: exp = [[s R, t], [0, 1]]."""
    from scipy.linalg import expm
    rng = np.random.default_rng(17)
    cases = [rng.normal(0, sc, 7) for sc in (1e-7, 1e-3, 0.3, 1.0) for _ in range(10)]
    cases += [np.r_[rng.normal(0, 0.5, 6), 0.0], np.r_[0, 0, 0, rng.normal(0, 0.5, 3), 0.4], np.r_[rng.normal(0, 0.5, 3), 0, 0, 0, 1e-7]]
    for u in cases:
        u = np.ascontiguousarray(u, np.float64)
        out = np.zeros(8)
        ref().sim3ref_exp(u.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        w = u[:3]
        G = np.zeros((4, 4))
        G[:3, :3] = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) + u[6] * np.eye(3)
        G[:3, 3] = u[3:6]
        E = expm(G)
        x, y, z, qw = out[:4]
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - qw * z), 2 * (x * z + qw * y)], [2 * (x * y + qw * z), 1 - 2 * (x * x + z * z), 2 * (y * z - qw * x)],
                      [2 * (x * z - qw * y), 2 * (y * z + qw * x), 1 - 2 * (x * x + y * y)]])
        assert np.allclose(out[7] * R, E[:3, :3], rtol=0, atol=1e-9), u
        # g2o takes C = 1 (and A, B without sigma) when |sigma| < 1e-5: a first-order term sigma / 2 * |upsilon| is dropped on purpose
        tol = 1e-9 + (abs(u[6]) * np.linalg.norm(u[3:6]) if abs(u[6]) < 1e-5 else 0.0)
        assert np.allclose(out[4:7], E[:3, 3], rtol=0, atol=tol), u
