"""The pose-only optimiser's case table (tests/pose_support.py) on the CPU oracle, no GPU: every case must reach the branch of
Optimizer::optimizePose (optimizer.cpp:358-501; k_pose_optimize in ydorbslam_amd/csrc/ba_kernels.hip.h, yo_pose_optimize in
oracle/ba_oracle.cpp) that it is in the table for, shown on the oracle's per-episode trace (oracle.orb_oracle.pose_optimize_trace),
and no classification in it may be a coin toss.  tests/test_pose_gpu.py then runs the same table through the kernel.

Branch -> case that reaches it (each asserted below):
  E < 3 exit (:443-445)                                   cut_0, cut_1, cut_2
  E < 10 exit after one episode (:494)                    cut_3, cut_9 (cut_10 is the first with four episodes)
  stride loops around kPoseThreads = 256                  cut_63 ... cut_513
  an episode with no active edge (nAct == 0)              no_active_edge, far_start_06 (episodes 1-3)
  a failed dense_solve<6>, the step applied anyway        zero_info (all 40 trials), nan_point
  the !isfinite(lambda) break                             nan_point, on the oracle only: the kernel's lambda_init drops the NaN (fmax)
  an excluded edge re-admitted after a later episode      cut_63, cut_64, cut_65, cut_255, cut_256, cut_257
  the switch to no robust kernel before episode 3         late_exclusion (an edge active in episode 3 ends beyond delta^2)
  ur == 0.0 is a stereo edge (not in the issue's list)     right_coordinate_zero
  the stale _error an active edge keeps after a rejected trial   every converging case: its episodes end on a rejected trial
"""
import numpy as np
import pytest

import pose_support as ps


@pytest.fixture(scope="module")
def traces(oracle_lib):
    return {k: oracle_lib.pose_optimize_trace(p) for k, p in ps.CASES.items()}


def _thresholds(prob):
    return np.where(prob["meas"][:, 2] >= 0, ps.TH_STEREO, ps.TH_MONO).astype(np.float32)


def test_every_case_states_its_purpose():
    assert set(ps.PURPOSE) == set(ps.CASES)
    assert [len(ps.CASES["cut_%d" % n]["info"]) for n in ps.CUT_COUNTS] == list(ps.CUT_COUNTS)
    assert max(len(p["info"]) for p in ps.CASES.values()) <= 600
    names, probs = ps.batch_order()
    assert len(names) == 2 * len(ps.CASES) and all(len(p["info"]) == 0 for n, p in zip(names, probs) if n is None)


def test_traced_entry_is_the_plain_entry(oracle_lib, traces):
    """yo_pose_optimize_trace runs yo_pose_optimize's body: the same bytes out, and a trace consistent with them."""
    for k, p in ps.CASES.items():
        r, t = oracle_lib.pose_optimize(p), traces[k]
        assert r["pose"].tobytes() == t["pose"].tobytes() and r["chi2"].tobytes() == t["chi2"].tobytes(), k
        assert r["inliers"] == t["inliers"] and r["trials"] == t["trials"] and np.array_equal(r["outlier"], t["outlier"]), k
        assert t["trials"] == t["epi_trials"].sum() and t["flag_trace"].shape == (t["episodes"], len(p["info"])), k
        assert np.array_equal(np.isfinite(t["chi2"]), t["epi_trials"] > 0) or k == "nan_point", k
        if t["episodes"]:
            assert np.array_equal(t["flag_trace"][-1], t["outlier"]) and t["inliers"] == len(p["info"]) - int(t["outlier"].sum()), k
            assert np.array_equal(t["flag_trace"], (t["chi_trace"] > _thresholds(p)).astype(np.uint8)), k


def test_edge_count_rules(traces):
    """E < 3: 0 returned, nothing touched (:443-445).  3 <= E < 10: one episode, so one finite chi2 and three NaN (:494).  E >= 10: four."""
    for n in ps.CUT_COUNTS:
        k = "cut_%d" % n
        t, p = traces[k], ps.CASES[k]
        if n < 3:
            assert t["inliers"] == 0 and t["trials"] == 0 and t["episodes"] == 0 and np.isnan(t["chi2"]).all(), k
            assert t["pose"].tobytes() == np.asarray(p["pose"], np.float64).tobytes(), k
        elif n < 10:
            assert t["episodes"] == 1 and np.isfinite(t["chi2"][0]) and np.isnan(t["chi2"][1:]).all() and t["epi_trials"][0] > 0, k
            assert (t["epi_trials"][1:] == 0).all() and t["epi_accepted"][0] > 0, k
        else:
            assert t["episodes"] == 4 and np.isfinite(t["chi2"]).all() and (t["epi_accepted"] > 0).all(), k
            assert t["chi2"][3] < t["chi2"][0] and 0.6 * n < t["inliers"] < n, k


def test_all_mono_and_all_stereo(traces):
    for k, stereo in (("all_mono", False), ("all_stereo", True)):
        p, t = ps.CASES[k], traces[k]
        assert len(p["info"]) == 40 and ((p["meas"][:, 2] >= 0) == stereo).all()
        assert t["episodes"] == 4 and 30 <= t["inliers"] < 40 and np.isfinite(t["chi2"]).all(), k


def test_zero_information(traces):
    """H + lambda I is the zero matrix: all 40 Cholesky factorisations fail, every trial applies the zero step and is rejected."""
    t, p = traces["zero_info"], ps.CASES["zero_info"]
    assert t["trials"] == 40 and list(t["epi_trials"]) == [10] * 4 and list(t["epi_failed_solves"]) == [10] * 4 and not t["epi_accepted"].any()
    assert (t["chi2"] == 0).all() and (t["chi_trace"] == 0).all() and t["inliers"] == 400 and not t["flag_trace"].any()
    assert t["pose"].tobytes() == ps.qnormalized(p["pose"]).tobytes()


@pytest.mark.parametrize("case", ["no_active_edge", "far_start_06"])
def test_no_active_edge_after_episode_0(traces, case):
    """Episode 0 runs its ten iterations (each accepted at its first trial) and its classification excludes every edge; episodes 1-3
    then have nAct == 0: no trial, NaN logged, and the pose they hand back is the start pose they were reset to (:455)."""
    t, p = traces[case], ps.CASES[case]
    assert list(t["epi_trials"]) == [10, 0, 0, 0] and t["trials"] == ps.FIXED_TRIALS[case] and t["epi_accepted"][0] == 10
    assert t["episodes"] == 4 and t["flag_trace"].all() and t["inliers"] == 0
    assert np.isfinite(t["chi2"][0]) and np.isnan(t["chi2"][1:]).all()
    assert t["pose"].tobytes() == ps.qnormalized(p["pose"]).tobytes()


def test_far_start_03_converges_like_the_near_start(traces):
    a, b = traces["far_start_03"], traces["near_start_002"]
    assert a["inliers"] == b["inliers"] == 256 and np.array_equal(a["outlier"], b["outlier"])
    assert np.allclose(a["pose"], b["pose"], rtol=0, atol=1e-6)


def test_readmission_and_late_exclusion(traces):
    """One case shows both: an edge flagged after episode 0 and clear at the end (the `fl & 1` refresh in the classification), and an
    edge clear after episode 0 and flagged at the end."""
    both = []
    for k, t in traces.items():
        if t["episodes"] == 4:
            ft = t["flag_trace"]
            readmitted, late = int(((ft[0] == 1) & (ft[3] == 0)).sum()), int(((ft[0] == 0) & (ft[3] == 1)).sum())
            if readmitted and late:
                both.append(k)
    print("re-admission and late exclusion in one run:", both)
    assert {"cut_63", "cut_64", "cut_65", "cut_255", "cut_256", "cut_257"} <= set(both)


def test_rank_deficient_geometry(traces):
    t = traces["rank_deficient"]
    assert t["episodes"] == 4 and t["trials"] <= 400 and t["inliers"] == 12 and np.isfinite(t["pose"]).all()
    assert not t["epi_failed_solves"].any() and t["chi2"][3] < 1e-12


def test_non_finite_input(traces):
    """One NaN point: every sum it enters is NaN.  The oracle keeps the NaN in lambda (std::max), fails its one Cholesky per episode
    and leaves through !isfinite(lambda); NaN > th is false, so the NaN edge is never flagged and stays active in all four episodes.
    Every other edge is classified by the error of the trial pose, which is the start pose (the failed solve left the step at zero)."""
    t, p = traces["nan_point"], ps.CASES["nan_point"]
    bad = int(np.flatnonzero(np.isnan(p["points"]).any(axis=1))[0])
    assert np.isnan(t["chi2"]).all() and list(t["epi_trials"]) == [1] * 4 and list(t["epi_failed_solves"]) == [1] * 4
    assert t["pose"].tobytes() == ps.qnormalized(p["pose"]).tobytes()
    assert not t["flag_trace"][:, bad].any() and np.isnan(t["chi_trace"][:, bad]).all()
    rest = np.arange(len(p["info"])) != bad
    start = ps.edge_chi2(p, ps.qnormalized(p["pose"]))[rest]
    th = _thresholds(p)[rest].astype(np.float64)
    assert (np.abs(start - th) > 1e-6 * th).all()                      # the numpy classification below is no coin toss either
    for e in range(4):
        assert np.array_equal(t["flag_trace"][e][rest], (start > th).astype(np.uint8))


def test_no_classification_is_a_coin_toss(traces):
    """Every case's flags are compared exactly with the kernel's, so no chi2 that a classification used may lie within a relative 1e-6
    of its threshold (the two sides differ by summation order, about 1e-12).  No case is exempt."""
    worst = {}
    for k, t in traces.items():
        if not t["chi_trace"].size:
            continue
        th = _thresholds(ps.CASES[k])
        rel = np.abs(t["chi_trace"] - th) / th
        assert not (rel <= 1e-6).any(), "%s: replace it by another seed" % k
        worst[k] = float(np.nanmin(rel))
    print("closest classification, relative distance from the threshold:", min(worst.items(), key=lambda kv: kv[1]))


def test_independent_reference_all_inlier_cases(traces):
    """No flag is ever set, so episode 3 runs without robust kernel over every edge and the oracle's chi2[3] is the plain cost
    sum info |z - pi(R X + t)|^2 at its returned pose (numpy, from the formulae of types_six_dof_expmap.h).  Bound: 16 x the
    difference between that expression in float64 and in longdouble (pose_support.cost_and_bound).  Also the sign convention of the
    pose update: the cost at the returned pose is below the cost at the start pose."""
    for k in ps.ALL_INLIER:
        p, t = ps.CASES[k], traces[k]
        assert not t["flag_trace"].any() and t["episodes"] == 4, k
        c64, cld, bound = ps.cost_and_bound(p, t["pose"])
        print("%s: numpy float64 %.17g, longdouble - float64 %.3e, bound %.3e, oracle chi2[3] - float64 %.3e"
              % (k, c64, float(cld - np.longdouble(c64)), bound, t["chi2"][3] - c64))
        assert bound > 0 and abs(t["chi2"][3] - c64) <= bound, k
        assert c64 < 0.1 * ps.reprojection_cost(p, ps.qnormalized(p["pose"])), k


def test_every_converging_case_lowers_the_independent_cost(traces):
    """Pose-update sign convention: wherever the oracle moved the pose, the numpy cost over its final inliers went down."""
    for k, t in traces.items():
        p = ps.CASES[k]
        if t["episodes"] == 0 or k in ps.START_POSE_RETURNED:
            continue
        keep = t["outlier"] == 0
        end, start = ps.edge_chi2(p, t["pose"])[keep].sum(), ps.edge_chi2(p, ps.qnormalized(p["pose"]))[keep].sum()
        assert end < start, (k, end, start)


def test_robust_kernel_is_off_in_episode_3(traces):
    """setRobustKernel(0) before the last episode (the `epi == 2` line): where an edge that episode 3 optimised over ends beyond its
    threshold (= Huber's delta^2), the logged chi2[3] is the plain sum over the edges active in episode 3 and not the Huber sum.
    1e-9 relative: each term is info r^2 with r a difference of ~300 px quantities, absolute error a few 1e-13 px, and the sums
    have at most 513 positive terms, so 1e-9 is far above both sides' rounding; the Huber sum must be off by more than a hundred times that (an edge just past its
    threshold changes it by (sqrt(chi2) - delta)^2 only)."""
    shown = []
    for k, t in traces.items():
        if t["episodes"] != 4 or not np.isfinite(t["chi2"][3]):
            continue
        p, ft = ps.CASES[k], t["flag_trace"]
        active = ft[2] == 0
        if not (active & (ft[3] == 1)).any():
            continue
        c = ps.edge_chi2(p, t["pose"])[active]
        d2 = np.where(p["meas"][active, 2] >= 0, 7.815, 5.991)
        huber = np.where(c <= d2, c, 2 * np.sqrt(c * d2) - d2)
        assert abs(t["chi2"][3] - c.sum()) <= 1e-9 * c.sum(), k
        assert abs(t["chi2"][3] - huber.sum()) > 1e-7 * c.sum(), k
        shown.append(k)
    print("late exclusion in episode 3:", shown)
    assert "late_exclusion" in shown


def test_right_coordinate_zero_is_a_stereo_edge(traces):
    """meas[2] >= 0 is the stereo test (the adapter writes -1 for ur < 0): an edge measured at ur == 0.0 exactly keeps its third
    residual.  Its classification chi2 is the three-dimensional numpy value (to float resolution), not the two-dimensional one."""
    p, t = ps.CASES["right_coordinate_zero"], traces["right_coordinate_zero"]
    assert p["meas"][0, 2] == 0.0 and (p["meas"][1:, 2] > 0).all()
    as_mono = dict(p)
    as_mono["meas"] = p["meas"].copy(); as_mono["meas"][0, 2] = -1.0
    c3, c2 = ps.edge_chi2(p, t["pose"])[0], ps.edge_chi2(as_mono, t["pose"])[0]
    assert abs(float(t["chi_trace"][-1][0]) - c3) <= 1e-6 * c3 and c3 - c2 > 1e-3 * c3, (t["chi_trace"][-1][0], c3, c2)


def test_episodes_end_on_a_rejected_trial(traces):
    """The stale _error: g2o's edges keep the error of the last computeActiveErrors, which after a rejected trial is that of the popped
    pose; the classification reads it for active edges.  Every converging case ends its last episode that way (the tail of no-op trials),
    at a step so small that float chi2 cannot tell - which is why only the flags, not this effect, can be asserted."""
    for k in ("cut_3", "cut_10", "cut_257", "cut_513", "all_mono", "all_stereo", "inliers_mixed_300"):
        t = traces[k]
        last = t["episodes"] - 1
        assert t["epi_last_rejected"][last] == 1 and t["epi_trials"][last] > t["epi_accepted"][last] > 0, k
