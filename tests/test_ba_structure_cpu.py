"""The inputs of the structure tests (tests/ba_support.py, second part) on the CPU oracle and the numpy references alone.

synth_ba_problem has information 1 on every edge, identity rotations, the same number of observations for every point, the fixed
keyframes first, no vertex without an edge, edges sorted by (point, pose) and every point in front of every camera.
realistic_ba_problem has none of these properties; the GPU parity tests (test_ba_structure_gpu.py) rely on what is asserted here:
the generator really has that structure, every row's oracle decisions are stable, the chi2 cull, the depth cull and a rejected step
really occur, and the two numpy references agree with the oracle - so a GPU mismatch cannot be blamed on the input or the reference.
"""
import numpy as np
import pytest

import ba_support as S

IDS = [r[0] for r in S.STRUCTURE_ROWS]


def test_generator_has_the_structure_it_promises():
    p = S.problem("R1")
    K, P, E = len(p["poses"]), len(p["points"]), len(p["edge_pose"])
    assert (K, P) == (14, 500) and list(np.flatnonzero(p["fixed"])) == [2, 5, 11]
    count = np.bincount(p["edge_point"], minlength=P)
    per_pose = np.bincount(p["edge_pose"], minlength=K)
    fixed_edge = p["fixed"][p["edge_pose"]] == 1
    stereo = p["meas"][:, 2] >= 0
    assert (count[:5] == 0).all() and (count[5:] >= 1).all()                              # 5 points without an edge
    free_obs = np.bincount(p["edge_point"][~fixed_edge], minlength=P)
    fixed_only = set(np.flatnonzero((count > 0) & (free_obs == 0)).tolist())
    assert set(range(5, 13)) <= fixed_only and len(fixed_only) <= 12                       # 8 points seen by fixed keyframes only (+ chance)
    single = np.flatnonzero(count == 1)
    assert set(range(13, 23)) <= set(single.tolist()) and not (set(range(13, 23)) & fixed_only)   # 10 points seen once, by a free keyframe
    assert all(stereo[p["edge_point"] == q].all() for q in single)                         # ... and every single observation is stereo
    assert len(set(count[23:])) >= 8 and count[23:].min() >= 2 and count[23:].max() == 13  # ragged, 2 .. every observing keyframe
    idle = np.flatnonzero(per_pose == 0)
    assert len(idle) == 1 and not p["fixed"][idle[0]]                                      # one free keyframe without an edge
    assert len(set(zip(p["edge_pose"].tolist(), p["edge_point"].tolist()))) == E           # one edge per (pose, point)
    key = p["edge_point"].astype(np.int64) * K + p["edge_pose"]
    assert 0.4 < np.mean(np.diff(key) < 0) < 0.6                                           # shuffled: half the neighbours descend
    assert np.array_equal(p["poses"][p["fixed"] == 1], p["truth_poses"][p["fixed"] == 1])  # fixed poses are not perturbed
    assert not np.isclose(p["poses"][p["fixed"] == 0], p["truth_poses"][p["fixed"] == 0]).all(axis=1).any()
    angle = 2 * np.arccos(np.clip(p["truth_poses"][:, 6], -1, 1))
    assert 0.55 < angle.max() < 0.75 and np.abs(p["truth_poses"][:, [3, 5]]).max() > 0.02  # up to ~0.6 rad about y, some about x and z
    assert np.array_equal(p["info"], (1.0 / 1.2 ** (2 * p["octave"])).astype(np.float32).astype(np.float64))
    assert set(p["octave"]) == set(range(8)) and len(set(p["info"])) == 8
    assert np.array_equal(p["meas"], p["meas"].astype(np.float32).astype(np.float64))
    assert 0.25 < np.mean(~stereo) < 0.40
    cam = p["camera"]
    assert cam[0] != cam[1] and not np.any(cam == np.round(cam)) and np.array_equal(cam, cam.astype(np.float32).astype(np.float64))
    assert (S.numpy_depths(p, p["truth_poses"], p["truth_points"]) > 2.0).all()
    again = S.realistic_ba_problem(seed=1)
    assert all(np.array_equal(again[k], p[k]) for k in p)                                  # seeded
    one = S.problem("one-free")
    assert len(one["poses"]) == 2 and list(one["fixed"]) == [1, 0] and (np.bincount(one["edge_pose"], minlength=2) > 0).all()
    assert S.problem("all-fixed")["fixed"].all()
    assert list(np.flatnonzero(S.problem("small-mid")["fixed"])) == [2]


@pytest.mark.parametrize("row", S.STRUCTURE_ROWS, ids=IDS)
def test_oracle_decisions_do_not_depend_on_rounding(oracle_lib, row):
    """As in test_ba_lm_paths_cpu.py: input perturbations of 1e-11 relative leave every integer decision alone and move chi2 by at
    most 1e-8 relative.  The all-fixed row holds at seed 1; where a generator change breaks a row, its seed changes, not this test."""
    _, name, spec = row
    stable, spread = S.decisions_are_stable(oracle_lib, S.problem(name), S.oracle_options(oracle_lib, spec))
    print("%s: stable %s, chi2 spread %.2e" % (row[0], stable, spread))
    assert stable
    assert spread <= 1e-8


def test_chi2_cull_fires_and_one_row_rejects_steps(oracle_lib):
    """Outlier share of every realistic row under the local schedule between 2 % and 20 % (4 % of the edges are 30 px off, and the
    octave noise puts more over the threshold); R5-far has an iteration with several trials.  Measured: 6.4 % .. 8.7 %; R5-far's
    third iteration takes 2 trials, every other row takes one trial per iteration."""
    rejecting = []
    for name in S.REALISTIC_ROWS:
        r = S.oracle_solve(oracle_lib, name, S.LOCAL)
        share = float(r["outlier"].mean())
        trials = S.trials_per_iteration(r["log"])
        print("%s: outliers %.1f %%, trials %s" % (name, 100 * share, trials))
        assert 0.02 < share < 0.20, name
        assert len(r["log"]) == 15 and set(r["log"][5:, 3]) == {2.0}, name               # both stages ran
        if max(trials) > 1:
            rejecting.append(name)
    assert "R5-far" in rejecting


@pytest.mark.parametrize("name", S.BACKFACING_ROWS)
def test_depth_cull_decides_the_backfacing_edges(oracle_lib, name):
    """All N_BACKFACING added edges are flagged, and for most of them the depth test is the ONLY reason: their chi2 at the returned
    estimate (numpy_chi2, per edge) is under the monocular threshold.  Measured: 12 of 12 under 5.991 with the camera fixed
    (largest 2.32) and 12 of 12 with it free (largest 2.90)."""
    p = S.problem(name)
    r = S.oracle_solve(oracle_lib, name, S.LOCAL)
    tail = slice(len(p["edge_pose"]) - S.N_BACKFACING, None)
    assert (p["edge_pose"][tail] == len(p["poses"]) - 1).all() and (p["meas"][tail, 2] < 0).all()
    assert r["outlier"][tail].all()
    depth = S.numpy_depths(p, r["poses"], r["points"])
    assert (depth[tail] < -1.0).all() and (depth[:tail.start] > 0).all()
    _, per_edge = S.numpy_chi2(p, r["poses"], r["points"], False, 0.0, 0.0)
    quiet = int((per_edge[tail] < 5.991).sum())
    print("%s: %d of %d back-facing edges have chi2 < 5.991 (%s)" % (name, quiet, S.N_BACKFACING, np.round(per_edge[tail], 2)))
    assert quiet >= 3
    base = S.oracle_solve(oracle_lib, "R2", S.LOCAL)                                         # the same problem without that keyframe
    assert r["outlier"][:tail.start].sum() <= base["outlier"].sum() + 5                      # ... is not disturbed by it


@pytest.mark.parametrize("robust", [True, False], ids=["robust", "plain"])
@pytest.mark.parametrize("name", ["R1", "R2", "back-free", "one-free", "all-fixed", "small", "small-mid"])
def test_numpy_chi2_agrees_with_the_oracle(oracle_lib, name, robust):
    """log[-1, 0] of a bundleAdjust-style solve is the objective at the estimate it returns.  Within 1e-8 with and without Huber,
    the deltas taken from the options in use.  Measured 3e-16 .. 4e-15: the intrinsics are float32 values, so the float baseline
    of g2o's cam_project costs nothing.  With localBundleAdjust's mono delta (sqrt(5.991)) against these options (sqrt(5.99)) the
    robust sums differ by about 2e-5, which the second assertion keeps visible."""
    p = S.problem(name)
    o = oracle_lib.ba_global_options(6, robust)
    r = S.oracle_solve(oracle_lib, name, ("global", 6, robust))
    total, per_edge = S.numpy_chi2(p, r["poses"], r["points"], robust, float(o["delta_mono"][0]), float(o["delta_stereo"][0]))
    rel = abs(total - r["log"][-1, 0]) / r["log"][-1, 0]
    print("%s %s: numpy %.12g oracle %.12g rel %.2e" % (name, "robust" if robust else "plain", total, r["log"][-1, 0], rel))
    assert rel <= 1e-8
    assert len(per_edge) == len(p["edge_pose"]) and (per_edge >= 0).all()
    if robust and name in ("R1", "R2"):
        local = oracle_lib.ba_default_options()
        other, _ = S.numpy_chi2(p, r["poses"], r["points"], True, float(local["delta_mono"][0]), float(local["delta_stereo"][0]))
        assert abs(other - r["log"][-1, 0]) / r["log"][-1, 0] > 1e-7


@pytest.mark.parametrize("name", S.SMALL_ROWS)
def test_numpy_lm_first_step_agrees_with_the_oracle(oracle_lib, name):
    """chi2 and lambda after ONE non-robust LM iteration: finite-difference Jacobians, dense H and numpy.linalg.solve against the
    oracle's analytic Jacobians, Schur complement and Cholesky.  Measured relative differences: chi2 1.1e-13 (small) and 5.0e-14
    (small-mid), lambda 1.6e-12 and 1.6e-12; one accepted trial on both.  Asserted with ten times the larger value.  A difference
    over 1e-6 would mean that the reference's retraction or lambda is not g2o's."""
    p = S.problem(name)
    r = S.oracle_solve(oracle_lib, name, S.GLOBAL1_N)
    chi2, lam, trials = S.numpy_lm_first_step(p)
    d_chi, d_lam = abs(chi2 - r["log"][0, 0]) / r["log"][0, 0], abs(lam - r["log"][0, 1]) / r["log"][0, 1]
    print("%s: chi2 numpy %.12g oracle %.12g rel %.2e; lambda numpy %.12g oracle %.12g rel %.2e" % (
        name, chi2, r["log"][0, 0], d_chi, lam, r["log"][0, 1], d_lam))
    assert len(r["log"]) == 1 and trials == int(r["log"][0, 2]) == 1
    assert chi2 < 0.5 * S.numpy_chi2(p, p["poses"], p["points"], False, 0.0, 0.0)[0]          # the step really moved the estimate
    assert d_chi <= S.LM_STEP_CHI2_RTOL and d_lam <= S.LM_STEP_LAMBDA_RTOL


def test_duplicated_edges_are_what_the_driver_refuses():
    """with_duplicated_edges repeats (pose, point) pairs and nothing else: the input of the GPU tests that expect YDORB_ERR_INVALID_ARG."""
    p = S.problem("R1")
    d = S.with_duplicated_edges(p, 10)
    pairs = list(zip(d["edge_pose"].tolist(), d["edge_point"].tolist()))
    assert len(pairs) == len(p["edge_pose"]) + 10 and len(set(pairs)) == len(p["edge_pose"])
    assert p["fixed"][d["edge_pose"][-10:]].any() and not p["fixed"][d["edge_pose"][-10:]].all()   # fixed and free poses among them
