"""GPU parity on inputs that make the LM loop reject steps (tests/ba_support.py; their properties are pinned on the CPU oracle in
test_ba_lm_paths_cpu.py).

Single solves against the oracle, with the tolerances of test_ba_gpu.py: a rejected trial, the estimate that stays put after it, the
chi2 recompute, termination on max_trials, a second stage with no edges left.  Lock-step batches whose members are out of phase - one
retries a rejected step while another starts an iteration, a third is in its second stage and a fourth is done - against their own
single solves, byte for byte.  And the batch with every upload of the round record delayed (YDORB_BA_TEST_LATE_UPLOADS), which
turns a host write into a pinned area whose copy is still in flight into a wrong result.
"""
import numpy as np
import pytest

import ba_support as S
from ydorbslam_amd.synth import synth_ba_problem

pytestmark = pytest.mark.gpu

IDS = [r[0] for r in S.STABLE_ROWS]
_single = {}


def single(name, spec):
    """The GPU's own single solve of a row: the reference of the batch tests (solves are bit reproducible), computed once."""
    import ydorbslam_amd as y
    if (name, spec) not in _single:
        _single[(name, spec)] = y.Optimizer.local_bundle_adjust(S.problem(name), S.gpu_options(spec))
    return _single[(name, spec)]


def _trial_lists_differ(solves):
    lists = {tuple(S.trials_per_iteration(r["log"])) for r in solves if len(r["log"])}
    return len(lists) > 1


@pytest.mark.parametrize("row", S.STABLE_ROWS, ids=IDS)
def test_single_solve_matches_oracle(oracle_lib, row):
    tag, name, spec = row
    ref = S.oracle_solve(oracle_lib, name, spec)
    got = single(name, spec)
    k = min(len(ref["log"]), len(got["log"]))
    rel = np.abs(got["log"][:k, :2] - ref["log"][:k, :2]) / np.abs(ref["log"][:k, :2])
    print("%s: trials gpu %s oracle %s; max rel chi2 %.2e lambda %.2e; outliers gpu %d oracle %d" % (
        tag, S.trials_per_iteration(got["log"]), S.trials_per_iteration(ref["log"]), rel[:, 0].max(), rel[:, 1].max(),
        int(got["outlier"].sum()), int(ref["outlier"].sum())))
    S.check_against_oracle(ref, got)
    if spec[0] == "global":
        assert set(got["log"][:, 3]) == {1.0}                                       # one stage only
    else:
        assert got["iterations"] == len(got["log"]) and not got["stopped"]


@pytest.mark.parametrize("row", [("C-local", "C", S.LOCAL), S.UNSTABLE_ROW], ids=["C-local", "G-local"])
def test_rejecting_solve_is_bit_reproducible_run_to_run(row):
    """Bit reproducibility does not need stable decisions, so G (a stage that ends early) serves here."""
    import ydorbslam_amd as y
    _, name, spec = row
    a = y.Optimizer.local_bundle_adjust(S.problem(name), S.gpu_options(spec))
    b = y.Optimizer.local_bundle_adjust(S.problem(name), S.gpu_options(spec))
    assert max(S.trials_per_iteration(a["log"])) >= 2
    assert S.same_bytes(a, b)
    assert S.same_bytes(a, single(name, spec))


@pytest.mark.parametrize("threads", [0, 2])
def test_lock_step_batch_with_members_out_of_phase(threads):
    """Members that reject at different iterations, one that ends after its first stage with every edge culled (F), one whose stage
    ends early (G), one that never rejects, one without edges and one whose stop flag is already set.  threads=2 advances them two at
    a time, which puts group boundaries between an early finisher and a late one."""
    import ydorbslam_amd as y
    names = ["A", "B", "C", "D", "F", "G"]
    plain = synth_ba_problem(4, 30, 3, seed=32)
    empty = dict(plain); empty["edge_pose"] = np.zeros(0, np.int32); empty["edge_point"] = np.zeros(0, np.int32)
    empty["meas"] = np.zeros((0, 3)); empty["info"] = np.zeros(0)
    probs = [S.problem(n) for n in names] + [plain, empty, S.problem("C")]
    stops = [None] * (len(probs) - 1) + [np.ones(1, np.uint8)]
    ref = [single(n, S.LOCAL) for n in names] + [y.Optimizer.local_bundle_adjust(plain), y.Optimizer.local_bundle_adjust(empty),
                                                   y.Optimizer.local_bundle_adjust(S.problem("C"), stop=np.ones(1, np.uint8))]
    assert _trial_lists_differ(ref)                                                  # else the batch was in lock step after all
    assert set(S.trials_per_iteration(ref[6]["log"])) == {1} and ref[7]["trials"] == 0
    batch = y.Optimizer.local_bundle_adjust_batch(probs, threads=threads, stops=stops)
    for i, (a, b) in enumerate(zip(ref, batch)):
        assert S.same_bytes(a, b), "member %d" % i
    last = batch[-1]
    assert last["stopped"] and last["trials"] == 0 and len(last["log"]) == 0
    assert np.array_equal(last["poses"], S.problem("C")["poses"]) and np.array_equal(last["points"], S.problem("C")["points"])
    assert stops[-1][0] == 1


@pytest.mark.parametrize("names,spec", [(["A", "B", "D"], S.GLOBAL_N), (["A", "C", "E"], S.GLOBAL_R), (["A", "C"], S.LOCAL_2)],
                         ids=["global-plain", "global-robust", "local-max2"])
def test_lock_step_batch_out_of_phase_with_other_options(names, spec):
    """bundleAdjust's single stage with and without the Huber kernels, and max_trials = 2 (a first stage that ends on the trial count)."""
    import ydorbslam_amd as y
    ref = [single(n, spec) for n in names]
    assert _trial_lists_differ(ref)
    batch = y.Optimizer.local_bundle_adjust_batch([S.problem(n) for n in names], S.gpu_options(spec))
    for n, a, b in zip(names, ref, batch):
        assert S.same_bytes(a, b), n


def test_lock_step_batch_with_late_uploads():
    """Every upload of the batch's round record waits 200 us on the stream before it reads its pinned source.  [B0, B0] is the
    all-in-step case: every round after the first builds the system without a host wait between the build's upload and the host's
    preparation of the trial's.  [A, C] adds rounds in which only some members build.  A build that saw the trial's flags would be
    skipped and the trial would run on the previous iteration's system."""
    import ydorbslam_amd as y
    from ydorbslam_amd._lib import BA_TEST_LATE_UPLOADS
    b0 = synth_ba_problem(5, 150, 4, seed=3)
    ref0 = y.Optimizer.local_bundle_adjust(b0)
    late = S.gpu_options(S.LOCAL, BA_TEST_LATE_UPLOADS)
    for i, b in enumerate(y.Optimizer.local_bundle_adjust_batch([b0, b0], late)):
        assert S.same_bytes(ref0, b), "B0 member %d: chi2 %s against %s" % (i, b["log"][:, 0], ref0["log"][:, 0])
    for n, b in zip("AC", y.Optimizer.local_bundle_adjust_batch([S.problem("A"), S.problem("C")], late)):
        a = single(n, S.LOCAL)
        assert S.same_bytes(a, b), "%s: chi2 %s against %s" % (n, b["log"][:, 0], a["log"][:, 0])
