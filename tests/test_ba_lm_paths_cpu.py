"""The inputs of tests/ba_support.py on the CPU oracle alone: they make the LM loop reject steps, and their decisions do not hang on
rounding.

The synthetic problems of the other BA tests take exactly one trial per outer iteration, all accepted, so a rejected step, the
chi2 recompute after one, termination on max_trials, a second stage without edges and a stage that ends early were never run.
The GPU parity tests (test_ba_lm_paths_gpu.py) rely on the properties asserted here; a change to synth.py that turns these inputs
back into all-accept runs fails here first.

Every row reproduced with the oracle as the Makefile builds it; no row was substituted.
"""
import numpy as np
import pytest

import ba_support as S

IDS = [r[0] for r in S.STABLE_ROWS]


@pytest.mark.parametrize("row", S.STABLE_ROWS, ids=IDS)
def test_oracle_decisions_do_not_depend_on_rounding(oracle_lib, row):
    """Input perturbations of 1e-11 relative leave every integer decision alone and move chi2 by at most 1e-8 relative: 100 times
    under the 1e-6 the GPU comparison allows."""
    _, name, spec = row
    stable, spread = S.decisions_are_stable(oracle_lib, S.problem(name), S.oracle_options(oracle_lib, spec))
    print("%s: stable %s, chi2 spread %.2e" % (row[0], stable, spread))
    assert stable
    assert spread <= 1e-8


@pytest.mark.parametrize("row", S.STABLE_ROWS, ids=IDS)
def test_rows_reject_steps(oracle_lib, row):
    tag, name, spec = row
    r = S.oracle_solve(oracle_lib, name, spec)
    trials = S.trials_per_iteration(r["log"])
    print("%s: trials %s (%d), stages %s, outliers %d/%d" % (tag, trials, r["trials"], [int(s) for s in r["log"][:, 3]],
                                                             int(r["outlier"].sum()), len(r["outlier"])))
    assert sum(trials) == r["trials"]
    if name == "F":
        # the first stage leaves every edge over the chi2 threshold: all culled, the second stage has nothing to optimise and logs nothing
        assert len(trials) == 5 and set(r["log"][:, 3]) == {1.0}
        assert r["outlier"].all()
        return
    assert max(trials) >= 2                                  # a rejected step, a retry with a larger lambda
    if name in ("A", "C", "E") and spec != S.LOCAL_2:
        assert max(trials) >= 4                              # several rejections in a row
    if spec == S.LOCAL_2:
        stage1 = r["log"][r["log"][:, 3] == 1]
        assert len(stage1) < 5 and stage1[-1, 2] == 2        # stage 1 ended by qmax == max_trials, not by its iteration count
        assert (r["log"][:, 3] == 2).any()


def test_unstable_row_is_unstable_and_ends_a_stage_early(oracle_lib):
    """G's decisions flip under a 1e-11 perturbation, so it cannot be compared with another implementation; it serves the GPU tests
    that compare the GPU with itself (run to run, batch against single).  Should it ever become stable it belongs in STABLE_ROWS."""
    _, name, spec = S.UNSTABLE_ROW
    r = S.oracle_solve(oracle_lib, name, spec)
    print("G: trials %s, stages %s, outliers %d/%d" % (S.trials_per_iteration(r["log"]), [int(s) for s in r["log"][:, 3]],
                                                       int(r["outlier"].sum()), len(r["outlier"])))
    assert len(r["log"]) < 15                                # a stage ends before its iteration count
    stable, _ = S.decisions_are_stable(oracle_lib, S.problem(name), S.oracle_options(oracle_lib, spec))
    assert not stable


def test_hard_problem_is_the_documented_perturbation():
    """hard_ba_problem draws the pose offsets first, then the point offsets, from default_rng(seed); fixed poses and rotations stay."""
    from ydorbslam_amd.synth import synth_ba_problem
    base = synth_ba_problem(5, 150, 4, seed=3)
    hard = S.hard_ba_problem(5, 150, 4, dict(seed=3), 1, 1.0, 2.0)
    rng = np.random.default_rng(1)
    dp = rng.normal(0, 1.0, (4, 3))
    dx = rng.normal(0, 2.0, (150, 3))
    assert np.array_equal(hard["poses"][0], base["poses"][0]) and np.array_equal(hard["poses"][:, 3:], base["poses"][:, 3:])
    assert np.array_equal(hard["poses"][1:, :3], base["poses"][1:, :3] + dp)
    assert np.array_equal(hard["points"], base["points"] + dx)
    for k in ("fixed", "edge_pose", "edge_point", "meas", "info", "camera"):
        assert np.array_equal(hard[k], base[k])
