"""GPU parity: HIP local BA (C ABI) vs the CPU oracle restatement of the g2o arithmetic.

Floating point: tolerance as BASELINE.md states it — poses/points |delta| <= 1e-4 relative on the float32 outputs,
robust chi2 trajectory within 1e-6 relative; the outlier mask (integer decisions) must be identical.
"""
import numpy as np
import pytest

from ba_support import check_against_oracle
from ydorbslam_amd.synth import synth_ba_problem

pytestmark = pytest.mark.gpu


def _check(prob, oracle_lib, options=None):
    import ydorbslam_amd as y
    ref = oracle_lib.ba_solve(prob)
    got = y.Optimizer.local_bundle_adjust(prob, options)
    check_against_oracle(ref, got)
    return ref, got


def test_small_stereo(oracle_lib):
    _check(synth_ba_problem(6, 120, 4, seed=3), oracle_lib)


def test_mono_stereo_mix_with_outliers(oracle_lib):
    prob = synth_ba_problem(20, 800, 8, seed=5, outlier_frac=0.05, mono_frac=0.4)
    ref, got = _check(prob, oracle_lib)
    assert 10 < ref["outlier"].sum() < 0.2 * len(ref["outlier"])                   # the chi2 cull really fires


def test_fixed_keyframes(oracle_lib):
    _check(synth_ba_problem(12, 400, 6, seed=7, n_fixed=4), oracle_lib)


def test_c5_shape(oracle_lib):
    """BASELINE config 5: 100 keyframes x 10 000 points, 8 observations each (80 000 stereo edges)."""
    prob = synth_ba_problem(100, 10000, 8, seed=1)
    ref, got = _check(prob, oracle_lib)
    assert got["log"][-1, 0] < 0.5 * got["log"][0, 0]
    # BA really moved the estimate toward the truth (free gauge: compare the chi2 instead of absolute error)


def test_stop_flag_and_empty(oracle_lib):
    import ydorbslam_amd as y
    prob = synth_ba_problem(6, 120, 4, seed=3)
    stop = np.ones(1, np.uint8)
    got = y.Optimizer.local_bundle_adjust(prob, stop=stop)
    assert got["stopped"] and got["trials"] == 0
    assert np.array_equal(got["poses"], prob["poses"]) and np.array_equal(got["points"], prob["points"])
    empty = dict(prob)
    empty["edge_pose"] = np.zeros(0, np.int32); empty["edge_point"] = np.zeros(0, np.int32)
    empty["meas"] = np.zeros((0, 3)); empty["info"] = np.zeros(0)
    got = y.Optimizer.local_bundle_adjust(empty)
    assert got["trials"] == 0


def test_dense_solve_known_answer(oracle_lib):
    """Reduced-system solver against numpy and against the SPD system pattern of g2o's linear_solver_test."""
    import ydorbslam_amd as y
    rng = np.random.default_rng(0)
    for n in (6, 36, 100, 594):
        M = rng.normal(size=(n, n))
        A = M @ M.T + n * np.eye(n)
        b = rng.normal(size=n)
        x, ok = y.Optimizer.dense_solve(A, b)
        assert ok
        assert np.allclose(x, np.linalg.solve(A, b), rtol=1e-9, atol=1e-12)
    A = np.eye(8); A[3, 3] = -1.0
    _, ok = y.Optimizer.dense_solve(A, np.ones(8))
    assert not ok   # not positive definite -> the LM step is rejected (linear_solver_eigen.h:118-126)


def test_concurrent_solves_use_separate_contexts(oracle_lib):
    """Several host threads may call ydorb_ba_solve at once (a pool of per-device contexts, one stream each); every kernel has a
    fixed summation order, so each concurrent solve must reproduce the sequential result bit for bit."""
    import threading
    import ydorbslam_amd as y
    from ydorbslam_amd.synth import synth_ba_problem
    probs = [synth_ba_problem(12 + 3 * i, 600 + 100 * i, 5, seed=40 + i) for i in range(4)]
    ref = [y.Optimizer.local_bundle_adjust(p) for p in probs]
    got = [None] * len(probs)

    def work(i):
        for _ in range(3):
            got[i] = y.Optimizer.local_bundle_adjust(probs[i])
    th = [threading.Thread(target=work, args=(i,)) for i in range(len(probs))]
    [t.start() for t in th]
    [t.join() for t in th]
    for r, g in zip(ref, got):
        assert g["trials"] == r["trials"]
        assert np.array_equal(g["outlier"], r["outlier"])
        assert g["poses"].tobytes() == r["poses"].tobytes() and g["points"].tobytes() == r["points"].tobytes()
        assert g["log"].tobytes() == r["log"].tobytes()


@pytest.mark.parametrize("robust", [True, False])
def test_global_bundle_adjust_single_stage(oracle_lib, robust):
    """Optimizer::bundleAdjust / globalBundleAdjust (optimizer.cpp:7-137, :353-357): same graph, ONE optimize(iterNum) call, no chi2
    cull, Huber optional with delta sqrt(5.99) — the §8(f) row that re-uses the local-BA kernels unchanged."""
    import ydorbslam_amd as y
    prob = synth_ba_problem(30, 2500, 6, seed=11, outlier_frac=0.03, mono_frac=0.3, n_fixed=1)
    ref = oracle_lib.ba_solve(prob, oracle_lib.ba_global_options(10, robust))
    got = y.Optimizer.local_bundle_adjust(prob, y.Optimizer.global_options(10, robust))
    assert got["trials"] == ref["trials"] and len(got["log"]) == len(ref["log"])
    assert set(got["log"][:, 3]) == {1.0}                                           # one stage only
    assert np.allclose(got["log"][:, :2], ref["log"][:, :2], rtol=1e-6, atol=0)
    assert np.array_equal(got["log"][:, 2:], ref["log"][:, 2:])
    assert np.array_equal(got["outlier"], ref["outlier"])
    assert np.allclose(got["poses"].astype(np.float32), ref["poses"].astype(np.float32), rtol=1e-4, atol=1e-6)
    assert np.allclose(got["points"].astype(np.float32), ref["points"].astype(np.float32), rtol=1e-4, atol=1e-6)
    two = y.Optimizer.local_bundle_adjust(prob)                                     # the two-stage schedule is a different run
    assert len(two["log"]) != len(got["log"]) or not np.allclose(two["log"][:, 0], got["log"][:, 0])


def test_pose_only_optimisation_batch(oracle_lib):
    """Optimizer::optimizePose (optimizer.cpp:358-501): one workgroup per frame runs all four episodes.
    Integer decisions (outlier flags, inlier count) must equal the oracle's; chi2 per episode within 1e-6, the pose within 1e-4
    relative on what Converter::transform_SE3_cvMat hands back as float.  The LM trial COUNT is not compared: once an episode has
    converged, chi2(current) - chi2(trial) is rounding noise (measured +-1e-12 of 1e3) and its sign decides accept / retry, so the
    tail of no-op trials differs with the summation order while every result stays the same."""
    import ydorbslam_amd as y
    from ydorbslam_amd.synth import synth_pose_problem
    probs = [synth_pose_problem(n, seed=50 + i, outlier_frac=o, mono_frac=m) for i, (n, o, m) in enumerate(
        [(400, 0.1, 0.3), (1000, 0.05, 0.0), (150, 0.3, 1.0), (9, 0.0, 0.5), (2, 0.0, 0.0), (2500, 0.15, 0.2), (40, 0.5, 0.5)])]
    got = y.Optimizer.optimize_poses(probs)
    for i, (p, g) in enumerate(zip(probs, got)):
        r = oracle_lib.pose_optimize(p)
        tag = "frame %d (E=%d): gpu chi2 %s oracle chi2 %s, inliers %d/%d, trials %d/%d" % (
            i, len(p["info"]), g["chi2"], r["chi2"], g["inliers"], r["inliers"], g["trials"], r["trials"])
        assert g["inliers"] == r["inliers"] and (g["trials"] > 0) == (r["trials"] > 0), tag
        assert np.array_equal(g["outlier"], r["outlier"]), tag
        assert np.array_equal(np.isnan(g["chi2"]), np.isnan(r["chi2"])), tag
        ok = ~np.isnan(r["chi2"])
        assert np.allclose(g["chi2"][ok], r["chi2"][ok], rtol=1e-6, atol=0), tag
        assert np.allclose(g["pose"].astype(np.float32), r["pose"].astype(np.float32), rtol=1e-4, atol=1e-6), tag + " pose %s vs %s" % (g["pose"], r["pose"])
    assert got[4]["inliers"] == 0 and np.array_equal(got[4]["pose"], probs[4]["pose"])      # < 3 correspondences: untouched
    one = y.Optimizer.optimize_poses(probs[:1])[0]                                            # batch position does not matter
    assert one["pose"].tobytes() == got[0]["pose"].tobytes() and np.array_equal(one["outlier"], got[0]["outlier"])


def test_solve_is_bit_reproducible_run_to_run():
    """Every reduction has a fixed order (pose-pair buckets are sorted by landmark up to 2048 observations per pose), so two
    solves of the same problem give identical bits - which is what lets kernel changes be checked for exact equality."""
    import ydorbslam_amd as y
    from ydorbslam_amd.synth import synth_ba_problem
    p = synth_ba_problem(30, 3000, 8, seed=4)
    a = y.Optimizer.local_bundle_adjust(p)
    b = y.Optimizer.local_bundle_adjust(p)
    assert a["poses"].tobytes() == b["poses"].tobytes() and a["points"].tobytes() == b["points"].tobytes()
    assert a["log"].tobytes() == b["log"].tobytes()


def test_batched_solve_equals_single_solves():
    """ydorb_ba_solve_batch: independent problems on pooled contexts, concurrently; each result identical to its own single solve."""
    import ydorbslam_amd as y
    from ydorbslam_amd.synth import synth_ba_problem
    probs = [synth_ba_problem(8 + 3 * i, 200 + 150 * i, 4 + i % 3, seed=20 + i, outlier_frac=0.05) for i in range(11)]
    single = [y.Optimizer.local_bundle_adjust(p) for p in probs]
    for threads in (0, 3):
        batch = y.Optimizer.local_bundle_adjust_batch(probs, threads=threads)
        for a, b in zip(single, batch):
            assert a["poses"].tobytes() == b["poses"].tobytes() and a["points"].tobytes() == b["points"].tobytes()
            assert np.array_equal(a["outlier"], b["outlier"]) and a["trials"] == b["trials"] and a["log"].tobytes() == b["log"].tobytes()
    assert y.Optimizer.local_bundle_adjust_batch([]) == []


def test_g2o_known_answer_system_through_the_hip_solver():
    """The reference's own solver fixture (thirdParty/g2o/unit_test/solver/sparse_system_helper.cpp, expected x checked with
    isApprox(1e-6) at linear_solver_test.cpp:69-83) fed through ydorb_ba_dense_solve — the k_chol_step / k_chol_solve chain the
    LM loop uses — with the original test's own tolerance.  This is the one reference-held vector on the BA path."""
    import json
    import os
    import ydorbslam_amd as y
    g = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g2o_linear_system.json")))
    A, b, x = np.array(g["A"]), np.array(g["b"]), np.array(g["x"])
    got, ok = y.Optimizer.dense_solve(A, b)
    assert ok
    assert np.linalg.norm(got - x) <= 1e-6 * min(np.linalg.norm(got), np.linalg.norm(x))   # Eigen isApprox(..., 1e-6)


@pytest.mark.parametrize("n", [1100, 2048, 4096])
def test_dense_solve_wider_than_one_workgroup(n):
    """Systems with more than 1024 rows (global BA with > 170 free keyframes): the backward substitution's column update is
    strided over the 1024-thread workgroup and y[n] needs the raised dynamic-LDS limit."""
    import ydorbslam_amd as y
    rng = np.random.default_rng(n)
    M = rng.normal(size=(n, n))
    A = M @ M.T + n * np.eye(n)
    b = rng.normal(size=n)
    x, ok = y.Optimizer.dense_solve(A, b)
    assert ok
    assert np.allclose(x, np.linalg.solve(A, b), rtol=1e-8, atol=1e-12)


def test_global_ba_with_more_than_200_free_keyframes(oracle_lib):
    """bundleAdjust over 230 keyframes (229 free -> a 1376-row reduced system, wider than the solve kernel's workgroup)."""
    import ydorbslam_amd as y
    prob = synth_ba_problem(230, 6000, 6, seed=13, outlier_frac=0.02, n_fixed=1)
    ref = oracle_lib.ba_solve(prob, oracle_lib.ba_global_options(4, True))
    got = y.Optimizer.local_bundle_adjust(prob, y.Optimizer.global_options(4, True))
    assert got["trials"] == ref["trials"] and len(got["log"]) == len(ref["log"])
    assert np.allclose(got["log"][:, :2], ref["log"][:, :2], rtol=1e-6, atol=0)
    assert np.array_equal(got["log"][:, 2:], ref["log"][:, 2:])
    assert np.array_equal(got["outlier"], ref["outlier"])
    assert np.allclose(got["poses"].astype(np.float32), ref["poses"].astype(np.float32), rtol=1e-4, atol=1e-6)
    assert np.allclose(got["points"].astype(np.float32), ref["points"].astype(np.float32), rtol=1e-4, atol=1e-6)


def test_stop_flag_set_from_another_thread_mid_solve():
    """Tracking flips LocalMapping's _bIsStopping while localBundleAdjust runs (tracking.cpp:786 -> localMapping.hpp:62); g2o
    polls it at the top of every iteration and inside the LM trial loop (sparse_optimizer.cpp:388,
    optimization_algorithm_levenberg.cpp:143) and optimizer.cpp:290 then skips the second stage.  A host thread sets the flag a few
    milliseconds into a C5 solve: the call must return early with stopped = 1 and hand back the last ACCEPTED estimate, i.e.
    exactly what an uninterrupted solve limited to that many iterations gives (every reduction has a fixed order, so bit for bit)."""
    import threading
    import time
    import ydorbslam_amd as y
    from ydorbslam_amd._lib import BA_SINGLE_STAGE
    prob = synth_ba_problem(100, 10000, 8, seed=1)
    full = y.Optimizer.local_bundle_adjust(prob)
    assert not full["stopped"] and full["iterations"] == 15
    seen = None
    for delay_ms in (3.0, 4.0, 2.0, 5.0, 6.0, 1.5, 7.0, 8.0, 1.0, 9.0, 10.0, 12.0, 14.0, 0.5):
        stop = np.zeros(1, np.uint8)

        def trip(d=delay_ms, s=stop):
            time.sleep(d * 1e-3)      # (a busy wait would hold the GIL for whole 5 ms switch intervals and starve the caller)
            s[0] = 1
        th = threading.Thread(target=trip)
        th.start()
        got = y.Optimizer.local_bundle_adjust(prob, stop=stop)
        th.join()
        if got["stopped"] and 0 < got["iterations"] < 15:
            seen = got
            break
    assert seen is not None, "no delay produced a mid-solve stop"
    k = seen["iterations"]
    assert seen["trials"] < full["trials"]
    assert np.array_equal(seen["log"][:k - 1], full["log"][:k - 1])            # the finished iterations are those of the full run
    stage = int(seen["log"][-1, 3])
    cands = []
    for j in (k, k - 1):                                                        # the interrupted iteration may have ended in a rejected trial
        o = y.Optimizer.default_options()
        if stage == 1:
            o.iters1, o.flags = j, BA_SINGLE_STAGE
        else:
            o.iters2 = j - 5
        if (stage == 1 and j >= 1) or (stage == 2 and j - 5 >= 0):
            cands.append(y.Optimizer.local_bundle_adjust(prob, o))
    assert any(c["poses"].tobytes() == seen["poses"].tobytes() and c["points"].tobytes() == seen["points"].tobytes() for c in cands)


def test_batch_with_mixed_sizes_empty_stopped_and_invalid_members(oracle_lib):
    """The lock-step batch takes problems of any size side by side, including ones that have nothing to do (no edges, stop flag already set)
    and invalid ones (reported per problem through rc_each, the others still solved); every solved member equals its single solve."""
    import ctypes as C
    import ydorbslam_amd as y
    from ydorbslam_amd._lib import YdBaProblem, YdBaResult, lib
    big = synth_ba_problem(40, 3000, 7, seed=31, outlier_frac=0.04, mono_frac=0.2)
    small = synth_ba_problem(4, 30, 3, seed=32)
    empty = dict(small); empty["edge_pose"] = np.zeros(0, np.int32); empty["edge_point"] = np.zeros(0, np.int32)
    empty["meas"] = np.zeros((0, 3)); empty["info"] = np.zeros(0)
    probs = [big, small, empty, synth_ba_problem(9, 300, 5, seed=33, n_fixed=3), small]
    stops = [None] * 4 + [np.ones(1, np.uint8)]                                      # the last member's stop flag is already set
    single = [y.Optimizer.local_bundle_adjust(p, stop=st) for p, st in zip(probs, stops)]
    batch = y.Optimizer.local_bundle_adjust_batch(probs, stops=stops)
    for a, b in zip(single, batch):
        assert a["poses"].tobytes() == b["poses"].tobytes() and a["points"].tobytes() == b["points"].tobytes()
        assert np.array_equal(a["outlier"], b["outlier"]) and a["trials"] == b["trials"] and a["log"].tobytes() == b["log"].tobytes()
    assert batch[2]["trials"] == 0
    assert batch[4]["stopped"] and batch[4]["trials"] == 0 and not batch[1]["stopped"]
    assert np.array_equal(batch[4]["poses"], small["poses"]) and np.array_equal(batch[4]["points"], small["points"])
    # global-BA options (single stage, no robust kernel) through the batch as well
    go = y.Optimizer.global_options(6, False)
    gs = [y.Optimizer.local_bundle_adjust(p, go) for p in probs[:2]]
    gb = y.Optimizer.local_bundle_adjust_batch(probs[:2], go)
    for a, b in zip(gs, gb):
        assert a["poses"].tobytes() == b["poses"].tobytes() and a["log"].tobytes() == b["log"].tobytes()
    # one invalid member (an edge that references a pose out of range): its rc is reported, the valid one is solved
    bad = dict(small); bad["edge_pose"] = small["edge_pose"].copy(); bad["edge_pose"][0] = 99
    L = lib()
    keep, P, R = [], (YdBaProblem * 2)(), (YdBaResult * 2)()
    for i, pr in enumerate((bad, small)):
        arrs = [np.ascontiguousarray(pr["poses"], np.float64).copy(), np.ascontiguousarray(pr["fixed"], np.uint8), np.ascontiguousarray(pr["points"], np.float64).copy(),
                np.ascontiguousarray(pr["edge_pose"], np.int32), np.ascontiguousarray(pr["edge_point"], np.int32), np.ascontiguousarray(pr["meas"], np.float64),
                np.ascontiguousarray(pr["info"], np.float64), np.zeros(len(pr["edge_pose"]), np.uint8)]
        keep.append(arrs)
        P[i] = YdBaProblem(len(arrs[0]), len(arrs[2]), len(arrs[3]), *[a.ctypes.data_as(C.c_void_p) for a in arrs[:7]], *[float(v) for v in pr["camera"]], None)
        R[i].edge_outlier = arrs[7].ctypes.data_as(C.c_void_p).value
    rc_each = (C.c_int32 * 2)()
    o = y.Optimizer.default_options()
    rc = L.ydorb_ba_solve_batch(P, 2, C.byref(o), R, 0, rc_each)
    assert rc != 0 and rc_each[0] != 0 and rc_each[1] == 0
    assert keep[1][0].tobytes() == single[1]["poses"].tobytes() and R[1].n_trials == single[1]["trials"]


@pytest.mark.parametrize("world", [2, 3])
def test_landmark_sharded_solve_through_the_allreduce_callback(world):
    """SURVEY 8(e), local BA on N GPUs: landmarks (and their edges) shard over ranks, every rank holds all poses, and the solver's five
    reduction points ([Hpp|bp], max diagonal, [S|bs], the step's scale terms, chi2) go through YdBaOptions.allreduce.  Here the ranks are
    host threads of ONE process on one GPU (each solve takes its own pooled context / stream) and the callback is a thread-barrier
    sum / max over the ranks' device comm buffers - what torch.distributed.all_reduce does over RCCL in bench.py.  The sharded solve
    must follow the unsharded one: same LM trial counts, chi2 / lambda trajectory to 1e-9 (the sums differ only in their association),
    identical outlier lists, poses equal on every rank, points equal shard by shard."""
    import threading
    import torch
    import ydorbslam_amd as y
    from ydorbslam_amd.parallel import shard_ba_problem
    prob = synth_ba_problem(12, 600, 6, seed=11, outlier_frac=0.04, mono_frac=0.3)
    ref = y.Optimizer.local_bundle_adjust(prob)
    dev = torch.device("cuda:0")
    ncomm = 128 * 129 + 4096
    comm = [torch.zeros(ncomm, dtype=torch.float64, device=dev) for _ in range(world)]
    bar = threading.Barrier(world)
    calls = [0] * world
    res, err = [None] * world, [None] * world

    def make_cb(r):
        def cb(user, d_buf, count, op):
            try:
                calls[r] += 1
                bar.wait(timeout=60)                 # every rank has copied its partial term into comm[r][:count]
                if r == 0:
                    parts = torch.stack([c[:count] for c in comm])
                    red = parts.max(dim=0).values if op == 1 else parts.sum(dim=0)
                    for c in comm:
                        c[:count].copy_(red)
                    torch.cuda.synchronize()
                bar.wait(timeout=60)
                return 0
            except Exception:  # noqa: BLE001
                return 1
        return cb

    def run(r):
        try:
            sub, _, _ = shard_ba_problem(prob, r, world)
            res[r] = y.Optimizer.local_bundle_adjust(sub, y.Optimizer.default_options(), allreduce=make_cb(r), comm_tensor_ptr=comm[r].data_ptr(),
                                                     comm_doubles=ncomm, rank=r, world=world)
        except Exception as e:  # noqa: BLE001
            err[r] = e
            bar.abort()
    ths = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=120)
    assert err == [None] * world, err
    assert len(set(calls)) == 1 and calls[0] > 5 * ref["trials"] // 2      # the reduction points were really exercised, equally on every rank
    for r in range(world):
        _, keep, ke = shard_ba_problem(prob, r, world)
        got = res[r]
        assert got["trials"] == ref["trials"] and np.array_equal(got["log"][:, 2:], ref["log"][:, 2:])
        assert np.allclose(got["log"][:, :2], ref["log"][:, :2], rtol=1e-9, atol=0)
        assert np.array_equal(got["outlier"], ref["outlier"][ke])
        assert np.allclose(got["poses"], ref["poses"], rtol=1e-9, atol=1e-12)
        assert np.array_equal(got["poses"], res[0]["poses"])              # every rank factorises the same reduced system
        assert np.allclose(got["points"], ref["points"][keep], rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("trip_at", [3, 8, 19])
def test_stop_flag_raised_at_a_fixed_reduction_is_deterministic(trip_at):
    """The asynchronous stop (tracking.cpp:786 -> localMapping.hpp:62) without a timer: the flag is raised inside the trip_at-th
    all-reduce callback of a 2-rank landmark-sharded solve, i.e. at the same point of the LM schedule on both ranks and in every run.
    The solve must end early with stopped = 1, both ranks must hold the same poses, and a second run must reproduce it bit for bit."""
    import threading
    import torch
    import ydorbslam_amd as y
    from ydorbslam_amd.parallel import shard_ba_problem
    prob = synth_ba_problem(12, 600, 6, seed=11, outlier_frac=0.04, mono_frac=0.3)
    full = y.Optimizer.local_bundle_adjust(prob)
    dev = torch.device("cuda:0")
    ncomm = 128 * 129 + 4096

    def sharded_run():
        comm = [torch.zeros(ncomm, dtype=torch.float64, device=dev) for _ in range(2)]
        bar = threading.Barrier(2)
        stop = np.zeros(1, np.uint8)
        calls = [0]
        res, err = [None, None], [None, None]

        def make_cb(r):
            def cb(user, d_buf, count, op):
                try:
                    bar.wait(timeout=60)
                    if r == 0:
                        calls[0] += 1
                        parts = torch.stack([c[:count] for c in comm])
                        red = parts.max(dim=0).values if op == 1 else parts.sum(dim=0)
                        for c in comm:
                            c[:count].copy_(red)
                        torch.cuda.synchronize()
                        if calls[0] == trip_at:
                            stop[0] = 1
                    bar.wait(timeout=60)
                    return 0
                except Exception:  # noqa: BLE001
                    return 1
            return cb

        def run(r):
            try:
                sub, _, _ = shard_ba_problem(prob, r, 2)
                res[r] = y.Optimizer.local_bundle_adjust(sub, y.Optimizer.default_options(), stop=stop, allreduce=make_cb(r),
                                                         comm_tensor_ptr=comm[r].data_ptr(), comm_doubles=ncomm, rank=r, world=2)
            except Exception as e:  # noqa: BLE001
                err[r] = e
                bar.abort()
        ths = [threading.Thread(target=run, args=(r,)) for r in range(2)]
        for t in ths:
            t.start()
        for t in ths:
            t.join(timeout=120)
        assert err == [None, None], err
        return res
    a, b = sharded_run(), sharded_run()
    for r in range(2):
        assert a[r]["stopped"] and a[r]["trials"] < full["trials"] and a[r]["iterations"] < full["iterations"]
        assert a[r]["poses"].tobytes() == b[r]["poses"].tobytes() and a[r]["points"].tobytes() == b[r]["points"].tobytes()
        assert a[r]["trials"] == b[r]["trials"]
    assert a[0]["poses"].tobytes() == a[1]["poses"].tobytes()


def test_release_gives_the_pooled_scratch_back():
    """ydorb_ba_release: the solver's pooled contexts (single solves, pose batches, lock-step batch jobs) free their device buffers and
    pinned staging; the next solve allocates again and gives the same result."""
    import torch
    import ydorbslam_amd as y
    prob = synth_ba_problem(20, 2000, 6, seed=2)
    a = y.Optimizer.local_bundle_adjust(prob)
    ba = y.Optimizer.local_bundle_adjust_batch([prob] * 3)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    y.Optimizer.release(0)
    free1 = torch.cuda.mem_get_info()[0]
    assert free1 > free0
    b = y.Optimizer.local_bundle_adjust(prob)
    bb = y.Optimizer.local_bundle_adjust_batch([prob] * 3)
    assert a["poses"].tobytes() == b["poses"].tobytes() and a["points"].tobytes() == b["points"].tobytes()
    assert all(x["poses"].tobytes() == a["poses"].tobytes() for x in ba + bb)


def test_result_does_not_depend_on_what_the_scratch_held():
    """A solve's device memory is a few arenas that are re-laid out in place for every problem, so a small problem solved after a
    large one runs on whatever the large one left there, at other offsets.  Problem B on freshly allocated arenas and B again on
    arenas that a larger problem A has just used must agree byte for byte - single solve, lock-step batch and pose-only batch -
    and the batch members must equal the single solve.  Anything a kernel reads before the stage has written it shows up here."""
    import ydorbslam_amd as y
    from ydorbslam_amd.synth import synth_pose_problem

    def run(prob, frames):
        return (y.Optimizer.local_bundle_adjust(prob), y.Optimizer.local_bundle_adjust_batch([prob, prob]),
                y.Optimizer.optimize_poses(frames))

    def same_ba(a, b):
        return (a["poses"].tobytes() == b["poses"].tobytes() and a["points"].tobytes() == b["points"].tobytes()
                and np.array_equal(a["outlier"], b["outlier"]) and a["trials"] == b["trials"] and a["log"].tobytes() == b["log"].tobytes())

    B = synth_ba_problem(5, 150, 4, seed=3)
    framesB = [synth_pose_problem(n_pts=60, seed=70 + i) for i in range(2)]
    A = synth_ba_problem(9, 600, 5, seed=4)
    framesA = [synth_pose_problem(n_pts=200, seed=80 + i) for i in range(4)]
    y.Optimizer.release(0)
    fresh = run(B, framesB)
    y.Optimizer.release(0)
    big = run(A, framesA)
    warm = run(B, framesB)
    for single, batch, _ in (fresh, big, warm):
        assert all(same_ba(single, m) for m in batch)
    assert same_ba(fresh[0], warm[0])
    assert all(same_ba(f, w) for f, w in zip(fresh[1], warm[1]))
    for f, w in zip(fresh[2], warm[2]):
        assert f["pose"].tobytes() == w["pose"].tobytes() and np.array_equal(f["outlier"], w["outlier"])
        assert f["inliers"] == w["inliers"] and f["trials"] == w["trials"] and f["chi2"].tobytes() == w["chi2"].tobytes()
