"""Essential-graph optimisation on the GPU (ydorb_essential_graph_optimize) against the CPU restatement tests/essgraph_ref and against
the generators' truth.  The tolerances come from essgraph_support.sensitivity / estimate_bounds."""
import functools

import numpy as np
import pytest

import essgraph_support as S

pytestmark = pytest.mark.gpu


def gpu_optimize(g, points=None, point_ref=None, **kw):
    from ydorbslam_amd.essential_graph import optimize_essential_graph
    return optimize_essential_graph(g["sim3"], g["fixed"], g["edges"], g["meas"], points, point_ref, fix_scale=g["fix_scale"], **kw)


@functools.lru_cache(maxsize=None)
def reference(shape, fix_scale):
    g = S.solve_graph(shape, fix_scale)
    return S.ref_optimize(g)


def check_linearize(g):
    from ydorbslam_amd.essential_graph import linearize_essential_graph
    ge, gj = S.sensitivity()
    got = linearize_essential_graph(g["sim3"], g["fixed"], g["edges"], g["meas"], fix_scale=g["fix_scale"])
    want = S.ref_linearize(g)
    de = float(np.abs(got["err"] - want["err"]).max())
    dj = max(float(np.abs(got["J0"] - want["J0"]).max()), float(np.abs(got["J1"] - want["J1"]).max()))
    print("%s fix_scale=%d: error gap %.3e (bound %.3e), Jacobian gap %.3e (bound %.3e)" % (g["name"], g["fix_scale"], de, S.MARGIN * ge, dj, S.MARGIN * gj))
    assert de <= S.MARGIN * ge
    assert dj <= S.MARGIN * gj
    assert np.abs(got["chi2"] - want["chi2"]).max() <= 2 * S.MARGIN * ge * np.sqrt(7 * want["chi2"].max()) + 1e-300
    fixed0, fixed1 = g["fixed"][g["edges"][:, 0]] != 0, g["fixed"][g["edges"][:, 1]] != 0
    assert not got["J0"][fixed0].any() and not got["J1"][fixed1].any()   # g2o does not differentiate with respect to a fixed vertex
    if g["fix_scale"]:
        assert not got["J0"][:, :, 6].any() and not got["J1"][:, :, 6].any()   # oplus drops update[6]: the column is exactly zero


def test_per_edge_errors_and_jacobians_in_every_log_branch():
    g = S.branch_graph()
    assert {S.log_branch(T) for T in S.edge_error_transforms(g)} == {0, 1, 2, 3}
    check_linearize(g)


@pytest.mark.parametrize("fix_scale", [True, False])
@pytest.mark.parametrize("shape", S.SOLVE_SHAPES)
def test_per_edge_kernel_on_the_solve_graphs(shape, fix_scale):
    check_linearize(S.solve_graph(shape, fix_scale))


@pytest.mark.parametrize("fix_scale", [True, False])
@pytest.mark.parametrize("shape", S.SOLVE_SHAPES)
def test_whole_solve_against_restatement_and_truth(shape, fix_scale):
    g = S.solve_graph(shape, fix_scale)
    want = reference(shape, fix_scale)
    got = gpu_optimize(g)
    between, to_truth = S.estimate_bounds(g, want["sim3"])
    between = min(between, 2 * to_truth)   # both within to_truth of the same point
    chi0 = S.ref_chi2(g, g["sim3"])
    d_ref, d_truth = S.distance(got["sim3"], want["sim3"]), S.distance(got["sim3"], g["truth"])
    k = S.iterations_above_noise(g, want["log_chi2"])
    print("%s fix_scale=%d: trials %s (restatement %s, %d above the noise), to restatement %.3e (bound %.3e), to truth %.3e (bound %.3e), "
          "chi2 %.3e -> %.3e" % (shape, fix_scale, got["log_trials"].tolist(), want["log_trials"].tolist(), k, d_ref, between, d_truth, to_truth, chi0,
                                 got["log_chi2"][-1]))
    # The accept / reject pattern.  Twenty iterations take every graph here down to the evaluation noise, where a trial is judged by the
    # sign of a difference of two noise-sized chi2 (iterations_above_noise has the threshold): that tail belongs to neither
    # implementation.  The pattern is compared where it is defined: the run of k iterations, whole, and the first k rows of the long one.
    assert k >= 1
    want_k, got_k = S.ref_optimize(g, iterations=k), gpu_optimize(g, iterations=k)
    assert got_k["log_trials"].tolist() == want_k["log_trials"].tolist()
    assert got_k["n_trials"] == want_k["n_trials"] and got_k["n_iterations"] == want_k["n_iterations"] == k
    assert got["log_trials"][:k].tolist() == want["log_trials"][:k].tolist()
    assert d_ref <= between
    # independent of both implementations: the generator's truth, and the chi2 the restatement's evaluator gives the GPU's estimates
    assert d_truth <= to_truth
    assert got["log_chi2"][-1] <= 1e-12 * chi0 and S.ref_chi2(g, got["sim3"]) <= 1e-12 * chi0
    fixed = g["fixed"] != 0
    assert np.array_equal(got["sim3"][fixed], g["sim3"][fixed])
    if fix_scale:   # the pivots of the scale rows are lambda alone, the factorisation still solves, and the scale never moves
        assert np.array_equal(got["sim3"][:, 7], g["sim3"][:, 7])


def apply_update(g, x):
    """oplus on the restatement: exp(x_f) * estimate for every free vertex"""
    est = np.array(g["sim3"], np.float64)
    for f, v in enumerate(np.nonzero(g["fixed"] == 0)[0]):
        est[v] = S.compose(S.sim3_exp(x[f]), est[v])
    return est


# the user lambda as the solve starts with it, and as twenty accepted trials can leave it (a third each time)
TRIAL_LAMBDAS = [1e-16, 1e-16 / 3.0 ** 20]


@pytest.mark.parametrize("lam", TRIAL_LAMBDAS)
@pytest.mark.parametrize("shape", S.SOLVE_SHAPES)
def test_fix_scale_trial_solves_and_its_scale_update_is_exactly_zero(shape, lam):
    """Under fix_scale column 6 of every Jacobian is exactly zero, so the scale rows of H + lambda I hold lambda alone.  The factorisation
    must still report a solve, and x[7f + 6] must be exactly 0 for every free vertex (b there is 0 and the factor's entries of those rows
    are products with 0): read from the trial's x itself, since oplus would drop update[6] whatever it held.  The rest of x is checked
    without either implementation's solver: it is finite, not zero, and applying it lowers the restatement's chi2."""
    from ydorbslam_amd.essential_graph import trial_step
    g = S.solve_graph(shape, True)
    x, solved = trial_step(g["sim3"], g["fixed"], g["edges"], g["meas"], lam, fix_scale=True)
    assert solved
    assert x.shape == (int((g["fixed"] == 0).sum()), 7) and np.isfinite(x).all()
    assert (x[:, 6] == 0.0).all(), x[:, 6]
    assert np.abs(x[:, :6]).max() > 1e-4
    assert S.ref_chi2(g, apply_update(g, x)) < 0.1 * S.ref_chi2(g, g["sim3"])


@pytest.mark.parametrize("shape", S.SOLVE_SHAPES)
def test_free_scale_trial_moves_the_scale(shape):
    from ydorbslam_amd.essential_graph import trial_step
    g = S.solve_graph(shape, False)
    x, solved = trial_step(g["sim3"], g["fixed"], g["edges"], g["meas"], 1e-16, fix_scale=False)
    assert solved and np.isfinite(x).all() and np.abs(x[:, 6]).max() > 1e-4
    assert S.ref_chi2(g, apply_update(g, x)) < 0.1 * S.ref_chi2(g, g["sim3"])


def test_fix_scale_solve_moves_the_estimate_and_keeps_the_scale():
    """One iteration, one trial on the six-vertex graph with fix_scale: the trial is accepted, the estimate moves, the scales stay."""
    g = S.solve_graph("six", True)
    got = gpu_optimize(g, iterations=1)
    assert got["log_trials"].tolist() == [1] and got["log_chi2"][0] < S.ref_chi2(g, g["sim3"])
    assert np.array_equal(got["sim3"][:, 7], g["sim3"][:, 7])
    assert S.distance(got["sim3"], g["sim3"]) > 1e-3


def chi2_gap_bound(g, chi):
    """|chi2 by the device - chi2 by the restatement| at one estimate: every error entry within MARGIN * g_e"""
    de = S.MARGIN * S.sensitivity()[0] * np.sqrt(7 * len(g["edges"]))
    return 2 * np.sqrt(chi) * de + de * de


def test_rejected_trial_pops_to_the_kept_estimate():
    g = S.far_start_graph()
    want = S.ref_optimize(g, **S.FAR)
    assert 1 < want["log_trials"][0] < 10   # the restatement rejects trials in its first iteration, then accepts one
    got = gpu_optimize(g, **S.FAR)
    print("far start: trials %s (restatement %s), chi2 %s (restatement %s)" % (got["log_trials"].tolist(), want["log_trials"].tolist(),
                                                                              got["log_chi2"].tolist(), want["log_chi2"].tolist()))
    assert got["log_trials"].tolist() == want["log_trials"].tolist() and got["n_trials"] == want["n_trials"]
    # every kept estimate lowers chi2, and what came back is the kept estimate: the restatement's evaluator gives it the logged chi2
    chi0 = S.ref_chi2(g, g["sim3"])
    assert got["log_chi2"][0] < chi0 and (np.diff(got["log_chi2"]) < 0).all()
    chi_back = S.ref_chi2(g, got["sim3"])
    assert abs(chi_back - got["log_chi2"][-1]) <= chi2_gap_bound(g, chi_back)
    # a run that ends in rejections only (one iteration, fewer trials than the first acceptance needs) hands the start back untouched
    k = int(want["log_trials"][0])
    stuck = gpu_optimize(g, iterations=1, max_trials=k - 1, lambda_init=S.FAR["lambda_init"])
    assert stuck["log_trials"].tolist() == [k - 1] and stuck["sim3"].tobytes() == np.ascontiguousarray(g["sim3"]).tobytes()


def test_two_calls_give_the_same_bytes():
    g = S.solve_graph("tree40", False)
    pts, ref = S.map_points(65, 40, 3)
    a, b = gpu_optimize(g, pts, ref), gpu_optimize(g, pts, ref)
    assert a["sim3"].tobytes() == b["sim3"].tobytes() and a["points"].tobytes() == b["points"].tobytes()
    assert a["log_chi2"].tobytes() == b["log_chi2"].tobytes() and a["log_lambda"].tobytes() == b["log_lambda"].tobytes()


def test_small_graph_after_a_large_one_reads_nothing_stale():
    from ydorbslam_amd.essential_graph import release
    release()
    small, large = S.solve_graph("six", True), S.solve_graph("tree40", False)
    first_small = gpu_optimize(small)
    first_large = gpu_optimize(large)
    again_small = gpu_optimize(small)
    again_large = gpu_optimize(large)
    assert again_small["sim3"].tobytes() == first_small["sim3"].tobytes() and again_small["log_chi2"].tobytes() == first_small["log_chi2"].tobytes()
    assert again_large["sim3"].tobytes() == first_large["sim3"].tobytes() and again_large["log_chi2"].tobytes() == first_large["log_chi2"].tobytes()
    release()
    assert gpu_optimize(small)["sim3"].tobytes() == first_small["sim3"].tobytes()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_map_point_correction(n):
    """points_out against the restatement's double result: one rounding to float, so within 1 float ulp of it (the two estimates differ
    far below a float ulp).  Point 0 hangs on the fixed vertex, whose estimate does not change: it comes back as it went in."""
    g = S.solve_graph("ring12", True)
    pts, ref = S.map_points(n, 12, 100 + n, always=(0,))
    want = S.ref_optimize(g, pts, ref)
    got = gpu_optimize(g, pts, ref)
    assert got["points"].shape == (n, 3) and got["points"].dtype == np.float32
    if n == 0:
        return
    ulp = np.spacing(np.abs(want["points_d"]).astype(np.float32)).astype(np.float64)
    assert (np.abs(got["points"].astype(np.float64) - want["points_d"]) <= ulp).all()
    assert np.array_equal(got["points"][0], pts[0])
    moved = ref != 0
    if moved.any():
        assert np.abs(got["points"][moved] - pts[moved]).max() > 1e-3   # the drifted keyframes' points do move
