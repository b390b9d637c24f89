"""The BA's block-skyline reduced camera solve on the GPU: the factorisation alone, one LM trial against the dense
path bit for bit, whole solves against the oracle and the dense path, maps above the dense limit, stale memory and control."""
import numpy as np
import pytest

import ba_skyline_support as K
import ba_support as S

pytestmark = pytest.mark.gpu

NATURAL, RCM, SMALLER = 1, 2, 0
AUTO, DENSE, SKYLINE = 0, 1, 2
OLD_TEXT = r"ydorb error -5: reduced camera system of \d+ rows is wider than the solve kernel's LDS \(max 19200\)"


def opt():
    import ydorbslam_amd as y
    return y.Optimizer


# ---- 1. the factorisation alone -------------------------------------------------------------------------------------------------------
def _star(n, hub):
    return [(hub, v) for v in range(n) if v != hub]


# k_sky_solve keeps a column's solved panel in LDS while its list has at most kSkyPanelLds = 128 rows (star129 hub first: 128, star130: 129)
# and strides its 1024 threads over panels of more than 1024 rows (star200 hub first: 1195)
PATTERNS = {
    "one": (1, []),
    "chain3": (3, K.ring(3, closed=False)),
    "ring12-open": (12, K.ring(12, closed=False)),
    "ring12": (12, K.ring(12)),
    "tree40": (40, K.tree40()),
    "star60-first": (60, _star(60, 0)),
    "star60-last": (60, _star(60, 59)),
    "components": (9, [(0, 1), (1, 2), (2, 0), (4, 5), (5, 6), (6, 7), (7, 8), (8, 4)]),      # block 3 on its own
    "banded-ring300": (300, K.banded_ring300()),
    "star129-first": (129, _star(129, 0)),
    "star130-first": (130, _star(130, 0)),
    "star200-first": (200, _star(200, 0)),
}


@pytest.mark.parametrize("ordering", [NATURAL, RCM])
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_factor_meets_the_backward_error_bound(name, ordering):
    """|| b - A x ||_2 <= n gamma_{3n+1} ||A||_2 ||x||_2 in long double, the condition-free bound of section 6j.  The measured ratios are in
    DESIGN.md section 6k; the bound is not tightened to them."""
    n, pairs = PATTERNS[name]
    A, b = K.block_spd(n, pairs, seed=len(pairs) + n)
    x, ok = opt().skyline_solve(A, b, ordering=ordering)
    assert ok and np.isfinite(x).all()
    holds, ratio, factor = K.residual_bound_ok(A, b, x)
    print("%s ordering %d: |r| / (|A| |x|) = %.3e, bound %.3e" % (name, ordering, ratio, factor))
    assert holds, (ratio, factor)
    xd, okd = opt().dense_solve(A, b)
    assert okd and np.allclose(x, xd, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("ordering", [NATURAL, RCM])
def test_factor_reports_a_block_that_is_not_spd(ordering):
    A, b = K.block_spd(12, K.ring(12), seed=3, bad_block=5)
    x, ok = opt().skyline_solve(A, b, ordering=ordering)
    assert not ok
    A, b = K.block_spd(12, K.ring(12), seed=3)
    assert opt().skyline_solve(A, b, ordering=ordering)[1]


# ---- 2. one trial ---------------------------------------------------------------------------------------------------------------------
_problems = {}


def problem(name):
    if name not in _problems:
        if name == "chain40":
            p = K.trajectory_problem(40, per_kf=6, seed=1)
        elif name == "loop40":
            p = K.trajectory_problem(40, per_kf=6, loop=True, seed=1)
        elif name == "synthA":
            from ydorbslam_amd.synth import synth_ba_problem
            p = synth_ba_problem(20, 800, 8, seed=5, outlier_frac=0.03, mono_frac=0.3)
        elif name == "synthB":
            from ydorbslam_amd.synth import synth_ba_problem
            p = synth_ba_problem(12, 300, 5, seed=7, n_fixed=2, outlier_frac=0.05, mono_frac=0.5)
        else:
            return S.problem(name)
        for v in p.values():
            v.setflags(write=False)
        _problems[name] = p
    return _problems[name]


TRIAL_PROBLEMS = ["A", "B", "E", "R1", "back-free", "one-free", "small", "small-mid", "chain40", "loop40"]


@pytest.mark.parametrize("name", TRIAL_PROBLEMS)
def test_one_trial_equals_the_dense_path_bit_for_bit(name):
    """Same sums in the same order, only the destination differs; RCM moves poses, so some blocks are stored transposed.  The solve of
    each solver meets the bound of the factor test; a lambda that makes the first pivot negative is an unsolved trial on both."""
    prob = problem(name)
    o = S.gpu_options(S.GLOBAL_R)
    scale = float(np.abs(np.diag(opt().reduced_system(prob, 0.0, o, solver=DENSE)["S"])).max())
    for lam in (1e-16 * scale, 1.0):
        dense = opt().reduced_system(prob, lam, o, solver=DENSE)
        n = len(dense["bs"])
        assert dense["solved"] and n % 6 == 0 and n > 0 and np.array_equal(dense["S"], dense["S"].T) and np.isfinite(dense["S"]).all()
        runs = {"dense": dense}
        for ordering in (NATURAL, RCM):
            sky = opt().reduced_system(prob, lam, o, solver=SKYLINE, ordering=ordering)
            assert sky["solved"]
            assert sky["S"].tobytes() == dense["S"].tobytes(), ordering
            assert sky["bs"].tobytes() == dense["bs"].tobytes(), ordering
            runs["skyline-%d" % ordering] = sky
        for tag, r in runs.items():
            holds, ratio, factor = K.residual_bound_ok(r["S"], r["bs"], r["x"])
            print("%s lambda %.3g %s: |r| / (|A| |x|) = %.3e, bound %.3e" % (name, lam, tag, ratio, factor))
            assert holds, (tag, ratio, factor)
    for kw in (dict(solver=DENSE), dict(solver=SKYLINE, ordering=NATURAL), dict(solver=SKYLINE, ordering=RCM)):
        assert not opt().reduced_system(prob, -1e6 * max(scale, 1.0), o, **kw)["solved"]


def test_rcm_stores_blocks_transposed():
    """the precondition of the transposed store in the test above: RCM reverses at least one covisible pair of loop40"""
    prob = problem("loop40")
    plan = opt().plan(prob, solver=SKYLINE, ordering=RCM)
    inv = np.argsort(plan["perm"])
    assert any(inv[a] > inv[b] for a, b in K.numpy_pairs(prob))


# ---- 3. whole solves below the limit --------------------------------------------------------------------------------------------------
SOLVE_ROWS = [(n, s) for n in ("chain40", "loop40", "synthA", "synthB") for s in (S.LOCAL, S.GLOBAL_R, S.GLOBAL_N)]
_oracle = {}


def oracle_solve(oracle_lib, name, spec):
    if (name, spec) not in _oracle:
        _oracle[(name, spec)] = oracle_lib.ba_solve(problem(name), S.oracle_options(oracle_lib, spec))
    return _oracle[(name, spec)]


@pytest.mark.parametrize("row", SOLVE_ROWS, ids=["%s-%s" % (n, "-".join(map(str, s))) for n, s in SOLVE_ROWS])
def test_whole_solve_against_oracle_and_dense(oracle_lib, row):
    name, spec = row
    prob = problem(name)
    if name in ("chain40", "synthB"):      # the precondition, kept cheap: the seeds were chosen with it on every row
        stable, _ = S.decisions_are_stable(oracle_lib, prob, S.oracle_options(oracle_lib, spec), n=2)
        assert stable
    ref = oracle_solve(oracle_lib, name, spec)
    dense = opt().local_bundle_adjust(prob, S.gpu_options(spec), solver=DENSE)
    old = opt().local_bundle_adjust(prob, S.gpu_options(spec))
    assert S.same_bytes(dense, old) and dense["info"]["solver_used"] == DENSE and old["info"] is None
    auto = opt().local_bundle_adjust(prob, S.gpu_options(spec), solver=AUTO)
    assert S.same_bytes(auto, old) and auto["info"]["solver_used"] == DENSE
    for ordering in (NATURAL, RCM):
        sky = opt().local_bundle_adjust(prob, S.gpu_options(spec), solver=SKYLINE, ordering=ordering)
        assert sky["info"]["solver_used"] == SKYLINE and sky["info"]["ordering_used"] == ordering
        S.check_against_oracle(ref, sky)
        S.check_against_oracle(dense, sky)
        again = opt().local_bundle_adjust(prob, S.gpu_options(spec), solver=SKYLINE, ordering=ordering)
        assert S.same_bytes(sky, again)


# ---- 4. above the limit, with a reference ---------------------------------------------------------------------------------------------
N_COPIES = 65


def copy_problem():
    return K.trajectory_problem(51, per_kf=4, seed=3, noise_px=1.0)


def test_disjoint_copies_above_the_limit_follow_the_oracle_of_one_copy(oracle_lib):
    """65 copies of a 51-keyframe problem (50 free each: 3 250 free keyframes, 19 500 rows).  chi2 is 65 times one copy's and the largest
    diagonal entry is one copy's, so the oracle's solve of one copy is the reference of every copy - as far as rho is one copy's too.
    It is not quite: rho = (chi2 - chi2') / (x . (lambda x + b) + 1e-3), and the 1e-3 does not grow with the copies.  lambda's factor
    max(1/3, min(1 - (2 rho - 1)^3, 2/3)) hides that wherever it is clamped, and shows it otherwise: the ORACLE's own lambda on two copies
    is then 2e-4 to 2e-2 off one copy's, and chi2 follows (measured here: with 8 iterations of this problem 65 copies on the GPU were
    1.7e-6 off in the sixth).  So the problem and the iteration count are chosen, with decisions_are_stable, such that every factor of
    the oracle's run is clamped, which is asserted as a precondition, together with the oracle's two-copy log against its one-copy log."""
    from ydorbslam_amd._lib import YdorbError
    one = copy_problem()
    spec = ("global", 4, True)
    stable, _ = S.decisions_are_stable(oracle_lib, one, S.oracle_options(oracle_lib, spec), n=2)
    assert stable
    ref = oracle_lib.ba_solve(one, S.oracle_options(oracle_lib, spec))
    factors = ref["log"][1:, 1] / ref["log"][:-1, 1]
    assert len(factors) == 3 and all(min(abs(f - 1 / 3), abs(f - 2 / 3)) < 1e-12 for f in factors), factors
    two = oracle_lib.ba_solve(K.copies(one, 2), S.oracle_options(oracle_lib, spec))
    assert np.allclose(two["log"][:, 0] / 2, ref["log"][:, 0], rtol=1e-12, atol=0) and np.allclose(two["log"][:, 1], ref["log"][:, 1], rtol=1e-12, atol=0)
    big = K.copies(one, N_COPIES)
    Kone, Pone, Eone = len(one["poses"]), len(one["points"]), len(one["edge_pose"])
    for kw in ({}, {"solver": DENSE}):
        with pytest.raises(YdorbError, match=OLD_TEXT):
            opt().local_bundle_adjust(big, S.gpu_options(spec), **kw)
    runs = [opt().local_bundle_adjust(big, S.gpu_options(spec), solver=s) for s in (SKYLINE, AUTO)]
    assert S.same_bytes(runs[0], runs[1])
    got = runs[1]
    assert got["info"]["solver_used"] == SKYLINE and got["info"]["n_free"] == 50 * N_COPIES and got["info"]["max_row_blocks"] <= 3
    assert got["trials"] == ref["trials"] and np.array_equal(got["log"][:, 2:], ref["log"][:, 2:])
    assert np.allclose(got["log"][:, 0] / N_COPIES, ref["log"][:, 0], rtol=1e-6, atol=0)
    assert np.allclose(got["log"][:, 1], ref["log"][:, 1], rtol=1e-6, atol=0)
    for c in range(N_COPIES):
        part = dict(trials=got["trials"], log=ref["log"], outlier=got["outlier"][c * Eone:(c + 1) * Eone],
                    poses=got["poses"][c * Kone:(c + 1) * Kone], points=got["points"][c * Pone:(c + 1) * Pone])
        S.check_against_oracle(ref, part)


# ---- 5. above the limit, connected ----------------------------------------------------------------------------------------------------
def _dof(prob):
    return 3 * len(prob["edge_pose"]) - 6 * int((K.free_index(prob) >= 0).sum()) - 3 * len(np.unique(prob["edge_point"]))


def test_connected_map_above_the_limit(oracle_lib):
    """A span-3 chain of 3 300 keyframes with one loop closure, 1 pixel of noise, global options.  No CPU reference fits (a dense LL^T of
    19 794 rows); the final chi2 per degree of freedom must agree with the oracle's on the same generator at 300 keyframes within three
    standard deviations of the two chi2-distributed statistics, sqrt(2 / dof) each, combined."""
    from ydorbslam_amd._lib import YdorbError
    spec = ("global", 5, True)
    big = K.trajectory_problem(3300, per_kf=4, loop=True, seed=12, noise_px=1.0)
    small = K.trajectory_problem(300, per_kf=4, loop=True, seed=11, noise_px=1.0)
    for kw in ({}, {"solver": DENSE}):
        with pytest.raises(YdorbError, match=OLD_TEXT):
            opt().local_bundle_adjust(big, S.gpu_options(spec), **kw)
    got = opt().local_bundle_adjust(big, S.gpu_options(spec), solver=AUTO)
    info = got["info"]
    assert info["solver_used"] == SKYLINE and info["ordering_used"] == RCM and info["n_free"] == 3299 and info["max_row_blocks"] <= 6
    chi = got["log"][:, 0]
    assert len(chi) >= 2 and (np.diff(chi) <= 0).all()
    ref = oracle_lib.ba_solve(small, S.oracle_options(oracle_lib, spec))
    dof_big, dof_small = _dof(big), _dof(small)
    a, b = chi[-1] / dof_big, ref["log"][-1, 0] / dof_small
    tol = 3 * np.sqrt(2.0 / dof_big + 2.0 / dof_small)
    print("chi2 / dof: 3 300 keyframes (GPU, skyline) %.5f over %d, 300 keyframes (oracle) %.5f over %d, tolerance %.5f" % (a, dof_big, b, dof_small, tol))
    assert abs(a - b) <= tol
    assert opt().local_bundle_adjust(big, S.gpu_options(spec), solver=SKYLINE)["poses"].tobytes() == got["poses"].tobytes()


# ---- 6. memory and control ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ordering", [NATURAL, RCM])
def test_small_solve_after_a_large_one_reads_nothing_stale(ordering):
    """The work arena is grow-only and keeps what earlier calls left: the small problem's envelope lies where the large one's factor lay."""
    small, large = problem("loop40"), K.trajectory_problem(400, per_kf=4, loop=True, seed=5)
    o = S.gpu_options(S.GLOBAL_R)
    opt().release()
    fresh = opt().local_bundle_adjust(small, o, solver=SKYLINE, ordering=ordering)
    big = opt().local_bundle_adjust(large, o, solver=SKYLINE, ordering=ordering)
    assert big["info"]["envelope_blocks"] > 5 * fresh["info"]["envelope_blocks"]
    after = opt().local_bundle_adjust(small, o, solver=SKYLINE, ordering=ordering)
    assert S.same_bytes(fresh, after)
    opt().release()
    assert S.same_bytes(fresh, opt().local_bundle_adjust(small, o, solver=SKYLINE, ordering=ordering))


def test_stop_flag_raised_before_the_call():
    prob = problem("chain40")
    stop = np.ones(1, np.uint8)
    got = opt().local_bundle_adjust(prob, S.gpu_options(S.LOCAL), stop=stop, solver=SKYLINE)
    assert got["stopped"] and got["trials"] == 0
    assert got["poses"].tobytes() == prob["poses"].tobytes() and got["points"].tobytes() == prob["points"].tobytes() and not got["outlier"].any()


def test_repeated_observations_are_still_refused():
    from ydorbslam_amd._lib import YdorbError
    prob = S.with_duplicated_edges(problem("chain40"), 3)
    for kw in (dict(solver=SKYLINE), dict(solver=AUTO), dict(solver=DENSE)):
        with pytest.raises(YdorbError, match="ydorb error -1: edges .* are both the observation of point"):
            opt().local_bundle_adjust(prob, S.gpu_options(S.LOCAL), **kw)
