"""The EPnP RANSAC's CPU side: setRansacParameters' arithmetic in the Python mirror against the restatement tests/pnp_ref, the
DESIGN.md section 2 ("EPnP RANSAC") linear algebra against numpy, noise-free EPnP known answers, iterate()'s loop rules on hand-built
cases, a degenerate quad, and the C++ adapter type-checked against the mocks."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from pnp_support import (K_VGA, ROOT, ref_eig_sym, ref_epnp, ref_lstsq, ref_params, ref_ransac, ref_svd, refine_fail_problem,
                         synth_problem, synth_scene)


@pytest.mark.parametrize("N,min_inl,eps", [(100, 10, 0.5), (10, 10, 0.5), (30, 8, 0.4), (7, 10, 0.5), (25, 10, 0.5), (1000, 10, 0.5),
                                           (12, 8, 0.4), (4, 4, 0.5)])
def test_ransac_parameters(N, min_inl, eps):
    from ydorbslam_amd.pnp import ransac_parameters
    got = ransac_parameters(N, 0.99, min_inl, 300, 4, eps)
    r = ref_params(N, 0.99, min_inl, 300, 4, eps)
    assert got[0] == r[0] and got[1] == r[1] and np.float32(got[2]) == np.float32(r[2])


def test_ransac_parameters_known_answers():
    from ydorbslam_amd.pnp import ransac_parameters
    assert ransac_parameters(10, 0.99, 10, 300, 4, 0.5)[:2] == (10, 1)              # minInliers == N: one iteration
    n_min, its, eps = ransac_parameters(30, 0.99, 8, 300, 4, 0.4)                   # N * eps = 12 > 8; ceil(log .01 / log(1 - .4^3))
    assert n_min == 12 and its == 70 and abs(eps - 0.4) < 1e-7
    n_min, its, eps = ransac_parameters(25, 0.99, 10, 300, 4, 0.2)                  # epsilon raised to 10 / 25
    assert n_min == 10 and np.float32(eps) == np.float32(10) / np.float32(25)
    assert its == int(np.ceil(np.log(0.01) / np.log(1 - np.float64(np.float32(0.4)) ** 3)))
    assert ransac_parameters(1000, 0.99, 10, 300, 4, 0.5)[:2] == (500, 35)


def test_symmetric_jacobi_against_numpy():
    rng = np.random.default_rng(1)
    for n in (3, 12):
        for _ in range(5):
            X = rng.normal(size=(n, n))
            A = X @ X.T
            d, ut = ref_eig_sym(A)
            w = np.linalg.eigvalsh(A)[::-1]
            assert np.allclose(d, w, rtol=0, atol=1e-13 * w[0])
            assert np.allclose(ut @ ut.T, np.eye(n), atol=1e-13)
            assert np.allclose(ut @ A @ ut.T, np.diag(d), atol=1e-12 * w[0])
            big = np.argmax(np.abs(ut), axis=1)
            assert np.all(ut[np.arange(n), big] > 0)                                   # sign normalisation


def test_one_sided_svd_and_lstsq_against_numpy():
    rng = np.random.default_rng(2)
    for m, k in ((6, 4), (6, 3), (6, 5), (3, 3)):
        for _ in range(5):
            A = rng.normal(size=(m, k))
            b = rng.normal(size=m)
            w, U, V = ref_svd(A)
            assert np.allclose(w, np.linalg.svd(A)[1], atol=1e-13)
            assert np.allclose(U @ np.diag(w) @ V.T, A, atol=1e-13)
            assert np.allclose(V.T @ V, np.eye(k), atol=1e-13)
            assert np.allclose(ref_lstsq(A, b), np.linalg.lstsq(A, b, rcond=None)[0], atol=1e-12)


@pytest.mark.parametrize("planar", [False, True])
@pytest.mark.parametrize("n", [4, 6, 100])
def test_noise_free_epnp_recovers_pose(n, planar):
    Xw, uv, R, t = synth_scene(n, 30 + n, planar=planar)
    Rr, tr, err = ref_epnp(Xw, uv, K_VGA)
    if planar and n == 4:   # the reference's EPnP has no planar branch: four coplanar points are not recovered
        return
    # the ABI's float inputs round the pixels by ~1e-5 px, which bounds the recovery
    tol = 1e-4 if n == 4 else 2e-6
    assert np.abs(Rr - R).max() < tol and np.linalg.norm(tr - t) / np.linalg.norm(t) < 10 * tol, (np.abs(Rr - R).max())
    assert err < 0.01


def _case(loop_or, max_its, n_hyp, min_inl, outliers=0.0):
    p, _, _ = synth_problem(40, 5, noise=0.0, outliers=outliers, min_inliers=4, n_hyp=n_hyp, loop_or=loop_or)
    p.update(min_inliers=min_inl, max_its=max_its)
    return p


def test_loop_condition_or_vs_and():
    # 90 % outliers against min_inliers 39: nothing qualifies, so the counts show how many hypotheses each loop rule runs
    for loop_or in (True, False):
        p = _case(loop_or, 7, 40, 39, outliers=0.9)
        r = ref_ransac(p, 5)
        assert r["ret_how"] == 0 and r["no_more"]
        if loop_or:   # one call runs max(maxIts, chunk) = 7
            assert r["next_hyp"] == 7 and r["n_calls"] == 1
        else:         # calls of 5 and 2
            assert r["next_hyp"] == 7 and r["n_calls"] == 2
        # a resumed call past maxIts: || runs chunk more, && runs none
        p.update(next_hyp=7)
        r = ref_ransac(p, 5)
        assert r["no_more"] and r["next_hyp"] == (12 if loop_or else 7)
        assert (r["hyp_inliers"] >= 0).sum() == (5 if loop_or else 0)


def test_refine_strict_threshold_then_success():
    # noise-free: every hypothesis counts all 40.  min_inliers 40: count >= 40 qualifies but Refine needs > 40 -> fails each time,
    # and the best pose comes back unrefined at exhaustion
    p = _case(False, 6, 40, 40)
    r = ref_ransac(p, 5)
    assert r["ret_how"] == 2 and r["ret_hyp"] == -1 and r["n_inliers"] == 40 and r["best_inliers"] == 40 and r["next_hyp"] == 6
    # 39: the first qualifying hypothesis refines to 40 > 39 and returns
    p = _case(False, 6, 40, 39)
    r = ref_ransac(p, 5)
    assert r["ret_how"] == 1 and r["ret_hyp"] == 0 and r["n_inliers"] == 40
    # a carried-in best mask of outlier matches: Refine on it fails at the first qualifying hypothesis and again at a second one that
    # does not beat the carried best (Refine's input unchanged); a later hypothesis beats the best and its Refine returns
    p, f, f2, h = refine_fail_problem()
    r = ref_ransac(p, 5)
    c, m, v = r["hyp_inliers"], p["min_inliers"], p["best_inliers"]
    assert f < f2 < h and m <= c[f] <= v and m <= c[f2] <= v and c[h] > v
    assert r["ret_how"] == 1 and r["ret_hyp"] == h and r["best_inliers"] == c[h] and r["n_inliers"] > m
    assert not np.array_equal(r["best_Tcw"], p["best_Tcw"])   # the best state moved to hypothesis h


def test_degenerate_quad_terminates_without_inliers():
    p, _, _ = synth_problem(20, 3, noise=0.0, min_inliers=4, n_hyp=3, loop_or=False)
    p["Xw"] = p["Xw"].copy()
    p["Xw"][[0, 1, 2, 3]] = p["Xw"][0]                   # a repeated point
    p["Xw"][[4, 5, 6, 7]] = np.float32([0, 0, 0])        # another one
    p["quads"] = np.array([[0, 1, 2, 3], [4, 5, 6, 7], [8, 8, 8, 8]], np.int32)
    p.update(min_inliers=4, max_its=3)
    r = ref_ransac(p, 5)
    assert np.all(r["hyp_inliers"] == 0) and r["ret_how"] == 0 and r["no_more"]
    R, t, err = ref_epnp(p["Xw"], p["P2D"], p["K"], [0, 1, 2, 3])
    assert not np.all(np.isfinite(np.concatenate([R.ravel(), t])))


def test_mirror_draw_and_sequence_length():
    from ydorbslam_amd.pnp import RandGen, draw_quads, sequence_length
    q = draw_quads(10, 50, RandGen(3))
    assert q.shape == (50, 4) and q.min() >= 0 and q.max() < 10
    assert all(len(set(row)) == 4 for row in q.tolist())
    assert sequence_length(100, 10, 35, 0, 5, True) == 35 and sequence_length(100, 10, 35, 33, 5, True) == 5
    assert sequence_length(100, 10, 35, 33, 5, False) == 2 and sequence_length(9, 10, 35, 0, 5, True) == 0


def test_one_iterate_call_draws_one_calls_worth():
    # iterate(5) is one call of the reference's loop: || runs until maxIts and 5 have run, && runs 5 or what maxIts leaves
    from ydorbslam_amd.pnp import PnPsolver, call_length
    assert call_length(100, 10, 35, 0, 5, True) == 35 and call_length(100, 10, 35, 40, 5, True) == 5
    assert call_length(100, 10, 35, 0, 5, False) == 5 and call_length(100, 10, 35, 33, 5, False) == 2
    assert call_length(100, 10, 35, 35, 5, False) == 0 and call_length(9, 10, 35, 0, 5, False) == 0
    p, _, _ = synth_problem(100, 4, outliers=0.3)
    s = PnPsolver(p["Xw"], p["P2D"], p["max_err"] / np.float32(5.991), p["K"])
    s.set_ransac_parameters(0.99, 10, 300, 4, 0.5, 5.991, loop_or=False)
    assert len(s.draw(5)) == 5
    s.set_ransac_parameters(0.99, 10, 300, 4, 0.5, 5.991, loop_or=True)
    assert len(s.draw(5)) == s.max_its > 5
    few = PnPsolver(p["Xw"][:3], p["P2D"][:3], np.ones(3, np.float32), p["K"])
    few.set_ransac_parameters(0.99, 3, 300, 3, 0.5, 5.991)   # minInliers 3 <= N = 3 < 4: no set of four can be drawn
    assert len(few.draw(5)) == 0


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_adapter_type_checks_against_mocks():
    inc = os.path.join(ROOT, "tests", "cpu_harness")
    src = os.path.join(ROOT, "tests", "cpu_harness", "pnp_syntax_check.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Wno-unused-parameter",
                           "-I", os.path.join(inc, "mockrt"), "-I", os.path.join(inc, "mock"), "-I", os.path.join(ROOT, "include"), src])
