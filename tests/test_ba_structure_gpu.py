"""GPU parity on graphs with realistic structure (tests/ba_support.py, second part; pinned on the CPU in test_ba_structure_cpu.py).

Every other BA test draws its input from synth_ba_problem: information 1 on every edge, identity rotations, the same number of
observations for every point, fixed keyframes first, no vertex without an edge, edges sorted by (point, pose), every depth
positive, at most 800 observations per pose.  A kernel that ignored the information, confused R with its transpose or never took
the depth branch of the cull, and a driver whose index maps only work near the identity, pass all of them.  Here: single solves
against the oracle; invariants that need no oracle (untouched vertices, the objective and the first LM iteration against numpy, the
depth rule); one, no and many observations per pose (the 2048-entry cap of k_pair_sort from both sides); the same edges in three
orders; all of it again through the lock-step batch; and problems that repeat a (pose, point) pair, which the driver refuses.
"""
import ctypes as C

import numpy as np
import pytest

import ba_support as S

pytestmark = pytest.mark.gpu

IDS = [r[0] for r in S.STRUCTURE_ROWS]
LOCAL_ROWS = S.REALISTIC_ROWS
GLOBAL_ROWS = [(n, s) for n in ("R1", "R2") for s in (S.GLOBAL6_R, S.GLOBAL6_N)] + [(n, S.GLOBAL6_R) for n in ("back-free", "one-free", "all-fixed")]
BATCH_ROWS = ["R1", "R2", "back-free", "one-free", "all-fixed", "cap-2048"]
_single = {}


def single(name, spec):
    """The GPU's own single solve of a row, computed once (solves are bit reproducible; callers must not write into it)."""
    import ydorbslam_amd as y
    if (name, spec) not in _single:
        _single[(name, spec)] = y.Optimizer.local_bundle_adjust(S.problem(name), S.gpu_options(spec))
    return _single[(name, spec)]


@pytest.mark.parametrize("row", S.STRUCTURE_ROWS, ids=IDS)
def test_single_solve_matches_oracle(oracle_lib, row):
    """The all-fixed row (no free pose: no pair bucket, a reduced system that is all padding) is compared in full: its oracle decisions
    are stable at the seed in use."""
    tag, name, spec = row
    ref = S.oracle_solve(oracle_lib, name, spec)
    got = single(name, spec)
    k = min(len(ref["log"]), len(got["log"]))
    rel = np.abs(got["log"][:k, :2] - ref["log"][:k, :2]) / np.abs(ref["log"][:k, :2])
    print("%s: trials gpu %s oracle %s; max rel chi2 %.2e lambda %.2e; outliers gpu %d oracle %d" % (
        tag, S.trials_per_iteration(got["log"]), S.trials_per_iteration(ref["log"]), rel[:, 0].max(), rel[:, 1].max(),
        int(got["outlier"].sum()), int(ref["outlier"].sum())))
    S.check_against_oracle(ref, got)
    if name in S.BACKFACING_ROWS:
        assert got["outlier"][-S.N_BACKFACING:].all()


def test_bucket_at_the_sort_cap_is_bit_reproducible():
    """3 keyframes, 2 of them free, 2048 points seen by all: every pair bucket has exactly kSortCap entries, the LDS key array of
    k_pair_sort is full and the bucket is still sorted, so the summation order is fixed.  (One point more and the bucket is copied
    unsorted: those rows are compared with the oracle only.)"""
    import ydorbslam_amd as y
    p = S.problem("cap-2048")
    assert (np.bincount(p["edge_pose"]) == 2048).all() and list(p["fixed"]) == [1, 0, 0]
    a = y.Optimizer.local_bundle_adjust(p)
    b = y.Optimizer.local_bundle_adjust(p)
    assert S.same_bytes(a, b) and S.same_bytes(a, single("cap-2048", S.LOCAL))


@pytest.mark.parametrize("name", LOCAL_ROWS)
def test_vertices_outside_the_system_come_back_untouched(name):
    p = S.problem(name)
    got = single(name, S.LOCAL)
    E = len(p["edge_pose"])
    assert len(got["outlier"]) == E and got["trials"] >= 15
    unobserved = np.bincount(p["edge_point"], minlength=len(p["points"])) == 0
    assert unobserved.sum() >= 2
    assert got["points"][unobserved].tobytes() == p["points"][unobserved].tobytes()          # bit for bit
    assert not np.array_equal(got["points"][~unobserved], p["points"][~unobserved])
    idle = (np.bincount(p["edge_pose"], minlength=len(p["poses"])) == 0) & (p["fixed"] == 0)
    assert idle.sum() == (0 if name in ("one-free", "all-fixed") else 1)
    still = (p["fixed"] == 1) | idle                                                         # the quaternion is normalised on the way in: float32
    assert np.array_equal(got["poses"][still].astype(np.float32), p["poses"][still].astype(np.float32))
    moved = ~still
    assert not np.isclose(got["poses"][moved], p["poses"][moved], rtol=0, atol=1e-9).all(axis=1).any()


@pytest.mark.parametrize("name,spec", GLOBAL_ROWS, ids=["%s-%s" % (n, "robust" if s[2] else "plain") for n, s in GLOBAL_ROWS])
def test_final_chi2_is_the_objective_at_the_returned_estimate(name, spec):
    """log[-1, 0] against numpy_chi2 (float64, no code shared with the oracle or the kernels) within the project's 1e-6: per-octave
    information, rotated cameras, both Huber deltas of the global path."""
    p = S.problem(name)
    got = single(name, spec)
    o = S.gpu_options(spec)
    total, _ = S.numpy_chi2(p, got["poses"], got["points"], spec[2], o.delta_mono, o.delta_stereo)
    rel = abs(total - got["log"][-1, 0]) / total
    print("%s %s: gpu %.12g numpy %.12g rel %.2e" % (name, spec, got["log"][-1, 0], total, rel))
    assert rel <= 1e-6
    ones = dict(p); ones["info"] = np.ones_like(p["info"])
    assert abs(S.numpy_chi2(ones, got["poses"], got["points"], spec[2], o.delta_mono, o.delta_stereo)[0] - total) / total > 0.1


@pytest.mark.parametrize("name", LOCAL_ROWS)
def test_every_edge_with_nonpositive_depth_is_flagged(name):
    """isDepthPositive at the returned estimate, with numpy's depths.  On the back-facing rows these are the added edges, whose chi2
    is small (test_ba_structure_cpu.py): only the depth term of k_cull can flag them."""
    p = S.problem(name)
    got = single(name, S.LOCAL)
    depth = S.numpy_depths(p, got["poses"], got["points"])
    behind = ~(depth > 0.0)
    print("%s: %d edges behind their camera, %d flagged" % (name, int(behind.sum()), int(got["outlier"].sum())))
    assert got["outlier"][behind].all()
    assert behind.sum() == (S.N_BACKFACING if name in S.BACKFACING_ROWS else 0)


@pytest.mark.parametrize("name", S.SMALL_ROWS)
def test_first_iteration_matches_the_numpy_lm_step(name):
    """chi2 and lambda after one non-robust iteration against numpy_lm_first_step: finite-difference Jacobians, dense normal
    equations.  Tolerance: the project's 1e-6 plus what that reference differs from the oracle by (ba_support.LM_STEP_*)."""
    chi2, lam, trials = S.numpy_lm_first_step(S.problem(name))
    got = single(name, S.GLOBAL1_N)
    print("%s: chi2 gpu %.12g numpy %.12g; lambda gpu %.12g numpy %.12g" % (name, got["log"][0, 0], chi2, got["log"][0, 1], lam))
    assert len(got["log"]) == 1 and got["trials"] == trials == 1
    assert abs(got["log"][0, 0] - chi2) <= (1e-6 + S.LM_STEP_CHI2_RTOL) * chi2
    assert abs(got["log"][0, 1] - lam) <= (1e-6 + S.LM_STEP_LAMBDA_RTOL) * lam


def test_edge_order_does_not_matter():
    """The same edges sorted by (point, pose) and in two seeded permutations: the driver orders them by (point, free-pose index,
    pose index) before anything is summed, so poses, points, trial count and log agree byte for byte, and the outlier masks agree
    once each permutation is undone."""
    import ydorbslam_amd as y
    p = S.problem("R1")
    E = len(p["edge_pose"])
    orders = [np.lexsort((p["edge_pose"], p["edge_point"]))] + [np.random.default_rng(s).permutation(E) for s in (7, 8)]
    solves = []
    for order in orders:
        q = dict(p)
        for k in ("edge_pose", "edge_point", "meas", "info"):
            q[k] = np.ascontiguousarray(p[k][order])
        r = y.Optimizer.local_bundle_adjust(q)
        mask = np.zeros(E, np.uint8)
        mask[order] = r["outlier"]                                                           # back to R1's own edge order
        solves.append((r, mask))
    ref, ref_mask = solves[0]
    assert 0 < ref_mask.sum() < E
    for r, mask in solves[1:]:
        assert r["poses"].tobytes() == ref["poses"].tobytes() and r["points"].tobytes() == ref["points"].tobytes()
        assert r["trials"] == ref["trials"] and r["log"].tobytes() == ref["log"].tobytes()
        assert np.array_equal(mask, ref_mask)
    assert np.array_equal(ref_mask, single("R1", S.LOCAL)["outlier"])                        # R1 itself is a fourth order


@pytest.mark.parametrize("threads", [0, 2])
def test_lock_step_batch_equals_the_single_solves(threads):
    """The kb_* kernels on the same index maps: two realistic problems, a back-facing camera, one free pose, no free pose and the
    full sort bucket side by side, each byte for byte its own single solve."""
    import ydorbslam_amd as y
    batch = y.Optimizer.local_bundle_adjust_batch([S.problem(n) for n in BATCH_ROWS], threads=threads)
    for n, b in zip(BATCH_ROWS, batch):
        assert S.same_bytes(single(n, S.LOCAL), b), n


# ---- duplicate (pose, point) edges: refused on the host ------------------------------------------------------------------------------
def _c_problems(probs):
    """YdBaProblem / YdBaResult arrays over private copies of the inputs; keep[i] = (poses, points, outlier) as the call leaves them."""
    from ydorbslam_amd._lib import YdBaProblem, YdBaResult
    n = len(probs)
    P, R, keep, hold = (YdBaProblem * n)(), (YdBaResult * n)(), [], []
    for i, pr in enumerate(probs):
        arrs = [np.ascontiguousarray(pr["poses"], np.float64).copy(), np.ascontiguousarray(pr["fixed"], np.uint8),
                np.ascontiguousarray(pr["points"], np.float64).copy(), np.ascontiguousarray(pr["edge_pose"], np.int32),
                np.ascontiguousarray(pr["edge_point"], np.int32), np.ascontiguousarray(pr["meas"], np.float64),
                np.ascontiguousarray(pr["info"], np.float64), np.zeros(len(pr["edge_pose"]), np.uint8)]
        hold.append(arrs)
        P[i] = YdBaProblem(len(arrs[0]), len(arrs[2]), len(arrs[3]), *[a.ctypes.data_as(C.c_void_p) for a in arrs[:7]], *[float(v) for v in pr["camera"]], None)
        R[i].edge_outlier = arrs[7].ctypes.data_as(C.c_void_p).value
        keep.append((arrs[0], arrs[2], arrs[7]))
    return P, R, keep, hold


INVALID_ARG = -1   # YDORB_ERR_INVALID_ARG


@pytest.mark.parametrize("name", ["R1", "all-fixed"])
def test_single_solve_refuses_duplicated_edges(name):
    """Ten (pose, point) pairs twice - fixed and free poses among them, all fixed on the second row: the invalid-argument code, the
    text names the pair, poses and points stay as they were.  The check runs in the host ordering, before any kernel."""
    import ydorbslam_amd as y
    from ydorbslam_amd._lib import YdorbError, lib
    bad = S.with_duplicated_edges(S.problem(name), 10)
    P, R, keep, _hold = _c_problems([bad])
    o = y.Optimizer.default_options()
    rc = lib().ydorb_ba_solve(C.byref(P[0]), C.byref(o), C.byref(R[0]))
    text = lib().ydorb_last_error().decode()
    print(rc, text)
    assert rc == INVALID_ARG and "observation of point" in text
    assert keep[0][0].tobytes() == np.ascontiguousarray(bad["poses"]).tobytes() and keep[0][1].tobytes() == np.ascontiguousarray(bad["points"]).tobytes()
    assert R[0].n_trials == 0 and not keep[0][2].any()
    with pytest.raises(YdorbError):
        y.Optimizer.local_bundle_adjust(bad, y.Optimizer.global_options(6, True))
    assert S.same_bytes(y.Optimizer.local_bundle_adjust(S.problem(name)), single(name, S.LOCAL))   # the context is as good as before


def test_sharded_solve_refuses_duplicated_edges():
    """world > 1 goes through the same host ordering: refused before the first collective, so a lone rank does not hang."""
    import ydorbslam_amd as y
    from ydorbslam_amd._lib import YdorbError
    calls = []

    def cb(user, d_buf, count, op):
        calls.append(count)
        return 1
    bad = S.with_duplicated_edges(S.problem("small"), 10)
    with pytest.raises(YdorbError, match="observation of point"):
        y.Optimizer.local_bundle_adjust(bad, y.Optimizer.default_options(), allreduce=cb, comm_tensor_ptr=None, comm_doubles=0, rank=0, world=2)
    assert calls == []


@pytest.mark.parametrize("threads", [0, 2])
def test_batch_reports_duplicated_edges_per_member(threads):
    """rc_each carries the code of the member with duplicates; its neighbours on both sides are solved, byte for byte as alone."""
    import ydorbslam_amd as y
    from ydorbslam_amd._lib import lib
    names = ["R2", None, "one-free", "small"]
    probs = [S.with_duplicated_edges(S.problem("R1"), 10) if n is None else S.problem(n) for n in names]
    P, R, keep, _hold = _c_problems(probs)
    rc_each = (C.c_int32 * len(probs))()
    o = y.Optimizer.default_options()
    rc = lib().ydorb_ba_solve_batch(P, len(probs), C.byref(o), R, threads, rc_each)
    assert rc == INVALID_ARG and list(rc_each) == [0, INVALID_ARG, 0, 0]
    assert keep[1][0].tobytes() == np.ascontiguousarray(probs[1]["poses"]).tobytes() and keep[1][1].tobytes() == np.ascontiguousarray(probs[1]["points"]).tobytes()
    for i, n in enumerate(names):
        if n is None:
            continue
        ref = single(n, S.LOCAL)
        assert keep[i][0].tobytes() == ref["poses"].tobytes() and keep[i][1].tobytes() == ref["points"].tobytes(), n
        assert np.array_equal(keep[i][2], ref["outlier"]) and R[i].n_trials == ref["trials"] and R[i].n_log == len(ref["log"]), n
        assert np.array_equal(np.array(R[i].log_chi2[:R[i].n_log]), ref["log"][:, 0]), n
