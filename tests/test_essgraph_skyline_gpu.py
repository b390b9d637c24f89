"""The essential graph's block-skyline solver on the GPU (ydorb_essential_graph_optimize_with / _trial_step_with):
the assembled system against the dense path's bit for bit, one trial against Higham's backward-error bound for a Cholesky solve, the
whole solve against the acceptance of test_essgraph_gpu.py, and a graph above the dense solver's limit against the skyline restatement
(tests/essgraph_ref/essgraph_skyline_ref.cpp)."""
import functools

import numpy as np
import pytest

import essgraph_skyline_support as K
import essgraph_support as S

pytestmark = pytest.mark.gpu


def gpu_optimize(g, points=None, point_ref=None, **kw):
    from ydorbslam_amd.essential_graph import optimize_essential_graph
    return optimize_essential_graph(g["sim3"], g["fixed"], g["edges"], g["meas"], points, point_ref, fix_scale=g["fix_scale"], **kw)


def gpu_trial(g, lam, **kw):
    from ydorbslam_amd.essential_graph import trial_step
    return trial_step(g["sim3"], g["fixed"], g["edges"], g["meas"], lam, fix_scale=g["fix_scale"], **kw)


@functools.lru_cache(maxsize=None)
def reference(shape, fix_scale):
    return S.ref_optimize(S.solve_graph(shape, fix_scale))


def same_result(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("sim3", "points", "log_chi2", "log_lambda", "log_trials")) and a["n_trials"] == b["n_trials"]


@pytest.mark.parametrize("fix_scale", [True, False])
@pytest.mark.parametrize("shape", S.SOLVE_SHAPES + ["ring12free"] + K.WIDE_SHAPES)
def test_assembled_system_equals_the_dense_path_bit_for_bit(shape, fix_scale):
    """Same sums in the same order, only the destination differs: H (without lambda, expanded, un-permuted) and b."""
    g = K.shape_graph(shape, fix_scale)
    _, solved, H, b = gpu_trial(g, 1.0, solver="dense", return_system=True)
    n = 7 * int((g["fixed"] == 0).sum())
    assert solved and H.shape == (n, n) and np.isfinite(H).all() and np.array_equal(H, H.T) and np.abs(H).max() > 0
    for ordering in ("natural", "rcm"):
        _, solved_s, Hs, bs = gpu_trial(g, 1.0, solver="skyline", ordering=ordering, return_system=True)
        assert solved_s
        assert Hs.tobytes() == H.tobytes(), ordering
        assert bs.tobytes() == b.tobytes(), ordering


U = 2.0 ** -53


@pytest.mark.parametrize("lam", [1e-16, 1.0])
@pytest.mark.parametrize("fix_scale", [True, False])
@pytest.mark.parametrize("shape", K.TRIAL_SHAPES)
def test_one_trial_meets_the_backward_error_bound_of_a_cholesky_solve(shape, fix_scale, lam):
    """r = b - (H + lambda I) x in long double; |r|_2 <= n gamma_{3n+1} |H + lambda I|_2 |x|_2 (Higham, Accuracy and Stability of Numerical
    Algorithms, theorem 10.4 with | |R^T| |R| |_2 <= n |A|_2): no condition number in it.  Asserted for the dense path too, so that the
    bound is seen to hold for the solver the project already trusts.  Measured ratios |r| / (|A| |x|): DESIGN.md section 6j."""
    g = K.shape_graph(shape, fix_scale)
    runs = {"dense": gpu_trial(g, lam, solver="dense", return_system=True)}
    for ordering in ("natural", "rcm"):
        runs[ordering] = gpu_trial(g, lam, solver="skyline", ordering=ordering, return_system=True)
    H, b = runs["dense"][2], runs["dense"][3]
    n = H.shape[0]
    A = H + lam * np.eye(n)
    norm_a = float(np.abs(np.linalg.eigvalsh(A)).max())   # symmetric: the 2-norm
    gamma = (3 * n + 1) * U / (1 - (3 * n + 1) * U)
    Al, bl = A.astype(np.longdouble), b.astype(np.longdouble)
    for name, (x, solved, Hr, br) in runs.items():
        assert solved, name
        assert Hr.tobytes() == H.tobytes() and br.tobytes() == b.tobytes()
        assert x.shape == (n // 7, 7) and np.isfinite(x).all() and np.abs(x).max() > 0
        r = bl - Al @ x.reshape(-1).astype(np.longdouble)
        res, norm_x = float(np.sqrt((r * r).sum())), float(np.linalg.norm(x))
        print("%s fix_scale=%d lambda=%g %s: n = %d, |r| / (|A| |x|) = %.3e, bound %.3e" % (shape, fix_scale, lam, name, n, res / (norm_a * norm_x), n * gamma))
        assert res <= n * gamma * norm_a * norm_x, name
        if fix_scale:   # the scale rows hold lambda alone: they factorise, and their update is exactly zero
            assert (x[:, 6] == 0.0).all(), name


@pytest.mark.parametrize("fix_scale", [True, False])
@pytest.mark.parametrize("shape", S.SOLVE_SHAPES)
def test_whole_solve_against_restatement_and_truth(shape, fix_scale):
    """The acceptance of test_essgraph_gpu.py's whole solve, for SKYLINE under SMALLER."""
    g = S.solve_graph(shape, fix_scale)
    want = reference(shape, fix_scale)
    got = gpu_optimize(g, solver="skyline", ordering="smaller")
    assert got["info"]["solver_used"] == "skyline" and got["info"]["n_free"] == int((g["fixed"] == 0).sum())
    between, to_truth = S.estimate_bounds(g, want["sim3"])
    between = min(between, 2 * to_truth)
    chi0 = S.ref_chi2(g, g["sim3"])
    d_ref, d_truth = S.distance(got["sim3"], want["sim3"]), S.distance(got["sim3"], g["truth"])
    k = S.iterations_above_noise(g, want["log_chi2"])
    print("%s fix_scale=%d (%s order): trials %s (restatement %s, %d above the noise), to restatement %.3e (bound %.3e), to truth %.3e (bound %.3e), "
          "chi2 %.3e -> %.3e" % (shape, fix_scale, got["info"]["ordering_used"], got["log_trials"].tolist(), want["log_trials"].tolist(), k, d_ref, between,
                                 d_truth, to_truth, chi0, got["log_chi2"][-1]))
    assert k >= 1
    want_k, got_k = S.ref_optimize(g, iterations=k), gpu_optimize(g, iterations=k, solver="skyline", ordering="smaller")
    assert got_k["log_trials"].tolist() == want_k["log_trials"].tolist()
    assert got_k["n_trials"] == want_k["n_trials"] and got_k["n_iterations"] == want_k["n_iterations"] == k
    assert got["log_trials"][:k].tolist() == want["log_trials"][:k].tolist()
    assert d_ref <= between
    assert d_truth <= to_truth
    assert got["log_chi2"][-1] <= 1e-12 * chi0 and S.ref_chi2(g, got["sim3"]) <= 1e-12 * chi0
    fixed = g["fixed"] != 0
    assert np.array_equal(got["sim3"][fixed], g["sim3"][fixed])
    if fix_scale:
        assert np.array_equal(got["sim3"][:, 7], g["sim3"][:, 7])


def test_rejected_trials_from_a_far_start():
    g = S.far_start_graph()
    want = S.ref_optimize(g, **S.FAR)
    for ordering in ("natural", "rcm"):
        got = gpu_optimize(g, solver="skyline", ordering=ordering, **S.FAR)
        assert got["log_trials"].tolist() == want["log_trials"].tolist() == [9, 1, 1] and got["n_trials"] == want["n_trials"]
        chi0 = S.ref_chi2(g, g["sim3"])
        assert got["log_chi2"][0] < chi0 and (np.diff(got["log_chi2"]) < 0).all()
        # cut off at eight trials, one short of the first acceptance: the start comes back byte for byte
        stuck = gpu_optimize(g, iterations=1, max_trials=8, lambda_init=S.FAR["lambda_init"], solver="skyline", ordering=ordering)
        assert stuck["log_trials"].tolist() == [8] and stuck["sim3"].tobytes() == np.ascontiguousarray(g["sim3"]).tobytes()


def test_map_point_correction():
    g = S.solve_graph("ring12", True)
    pts, ref = S.map_points(65, 12, 165, always=(0,))
    want = S.ref_optimize(g, pts, ref)
    got = gpu_optimize(g, pts, ref, solver="skyline", ordering="rcm")
    ulp = np.spacing(np.abs(want["points_d"]).astype(np.float32)).astype(np.float64)
    assert got["points"].shape == (65, 3) and (np.abs(got["points"].astype(np.float64) - want["points_d"]) <= ulp).all()
    assert np.array_equal(got["points"][0], pts[0]) and np.abs(got["points"][ref != 0] - pts[ref != 0]).max() > 1e-3


def test_two_calls_give_the_same_bytes():
    g = S.solve_graph("tree40", False)
    pts, ref = S.map_points(65, 40, 3)
    for ordering in ("natural", "rcm"):
        a, b = gpu_optimize(g, pts, ref, solver="skyline", ordering=ordering), gpu_optimize(g, pts, ref, solver="skyline", ordering=ordering)
        assert same_result(a, b), ordering


def test_small_graph_after_a_large_one_reads_nothing_stale():
    """The work arena is grow-only and keeps what earlier calls left: the envelope, b and x of the small graph lie where the large one's
    factor lay."""
    from ydorbslam_amd.essential_graph import release
    small, large = S.solve_graph("six", True), K.shape_graph("ring300", False)
    release()
    first_small = gpu_optimize(small, solver="skyline")
    release()
    first_large = gpu_optimize(large, solver="skyline", iterations=3)
    again_small = gpu_optimize(small, solver="skyline")
    again_large = gpu_optimize(large, solver="skyline", iterations=3)
    assert same_result(again_small, first_small) and same_result(again_large, first_large)
    # the wide shapes in natural order: rows and column lists longer than one pass of the workgroup, each after another shape's factor
    first = {}
    for shape in K.WIDE_SHAPES:
        release()
        first[shape] = gpu_optimize(K.shape_graph(shape, False), solver="skyline", ordering="natural", iterations=3)
        assert first[shape]["info"]["ordering_used"] == "natural" and first[shape]["info"]["max_row_blocks"] >= 60
    for shape in K.WIDE_SHAPES + K.WIDE_SHAPES[::-1]:
        assert same_result(gpu_optimize(K.shape_graph(shape, False), solver="skyline", ordering="natural", iterations=3), first[shape]), shape
        assert same_result(gpu_optimize(small, solver="skyline"), first_small), shape
    dense_small = gpu_optimize(small)   # and the dense path after the skyline one, in the same arena
    release()
    assert same_result(gpu_optimize(small), dense_small)


def test_non_positive_pivot_is_a_rejected_trial_not_an_error():
    """lambda = -1e6 makes the first pivot negative (the entries of H are of order 1e2).  The kernel replaces the pivot, walks on to its
    last barrier and reports the trial unsolved; the call returns YDORB_OK (no exception here), and the next call is untouched."""
    g = S.solve_graph("ring12", False)   # repeats the pair (3, 4)
    good = gpu_trial(g, 1e-16, solver="skyline", ordering="rcm")
    for ordering in ("natural", "rcm"):
        x, solved = gpu_trial(g, -1e6, solver="skyline", ordering=ordering)
        assert solved is False and x.shape == (11, 7)
    again = gpu_trial(g, 1e-16, solver="skyline", ordering="rcm")
    assert good[1] and again[1] and again[0].tobytes() == good[0].tobytes()


def test_entries_agree_on_the_dense_solver():
    g = S.solve_graph("tree40", True)
    pts, ref = S.map_points(40, 40, 9)
    old = gpu_optimize(g, pts, ref)
    dense, auto = gpu_optimize(g, pts, ref, solver="dense"), gpu_optimize(g, pts, ref, solver="auto")
    assert same_result(dense, old) and same_result(auto, old)
    assert dense["info"]["solver_used"] == auto["info"]["solver_used"] == "dense" and "info" not in old
    assert auto["info"]["envelope_blocks"] == min(auto["info"]["envelope_blocks_natural"], auto["info"]["envelope_blocks_rcm"])
    x_old, ok_old = gpu_trial(g, 1e-16)
    x_new, ok_new = gpu_trial(g, 1e-16, solver="dense")
    assert ok_old and ok_new and x_old.tobytes() == x_new.tobytes()


BIG_N = 3000


@functools.lru_cache(maxsize=None)
def big_graph():
    n = BIG_N
    edges = [(n - 1, 0)] + [(i, i - 1) for i in range(1, n)] + [(i, i - 2) for i in range(2, n)]
    g = S.make_graph(n, edges, 4000, True, drift=0.002, name="ring%d" % n)
    pts, ref = S.map_points(200, n, 17, always=(0,))
    return g, pts, ref, K.sky_ref_optimize(g, pts, ref, iterations=6)


def test_above_the_dense_limit():
    """3 000 keyframes: the dense solver and the old entry refuse, AUTO and SKYLINE solve.  estimate_bounds needs the singular values of a
    63 000 x 21 000 Jacobian, minutes of work, so the two checks the size allows stand in for it: the distance to the generator's truth
    against the skyline restatement's own, and chi2 (DESIGN.md section 6j has the measured figures)."""
    from ydorbslam_amd._lib import YdorbError
    g, pts, ref, want = big_graph()
    for kw in ({}, {"solver": "dense"}):
        with pytest.raises(YdorbError, match="ydorb error -5.*at most 2742"):
            gpu_optimize(g, pts, ref, iterations=6, **kw)
    chi0 = S.ref_chi2(g, g["sim3"])
    ref_truth = S.distance(want["sim3"], g["truth"])
    for solver in ("auto", "skyline"):
        got = gpu_optimize(g, pts, ref, iterations=6, solver=solver)
        info = got["info"]
        assert info["solver_used"] == "skyline" and info["n_free"] == BIG_N - 1 and info["factor_bytes"] == 392 * info["envelope_blocks"]
        d_truth, d_ref = S.distance(got["sim3"], g["truth"]), S.distance(got["sim3"], want["sim3"])
        print("ring%d %s: order %s, envelope %d blocks (natural %d, rcm %d), trials %s (restatement %s), chi2 %.3e -> %.3e (restatement %.3e), to truth "
              "%.3e (restatement %.3e), to restatement %.3e" % (BIG_N, solver, info["ordering_used"], info["envelope_blocks"], info["envelope_blocks_natural"],
                                                                 info["envelope_blocks_rcm"], got["log_trials"].tolist(), want["log_trials"].tolist(), chi0,
                                                                 got["log_chi2"][-1], want["log_chi2"][-1], d_truth, ref_truth, d_ref))
        assert d_truth <= 2 * ref_truth
        assert got["log_chi2"][-1] <= 1e-12 * chi0 and S.ref_chi2(g, got["sim3"]) <= 1e-12 * chi0
        ulp = np.spacing(np.abs(want["points_d"]).astype(np.float32)).astype(np.float64)
        assert got["points"].shape == (200, 3) and (np.abs(got["points"].astype(np.float64) - want["points_d"]) <= ulp).all()
        assert np.array_equal(got["points"][0], pts[0])
