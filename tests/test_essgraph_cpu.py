"""Essential-graph optimisation without a GPU: known answers of the CPU restatement (tests/essgraph_ref), the adapter's syntax check,
the ABI's argument checks (they return before any device work) and the sensitivity figures that set the GPU tests' tolerances."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import essgraph_support as S
from essgraph_support import ROOT

# one hand-picked u per branch of Sim3::log: (u, branch bits: 1 = |sigma| < 1e-5, 2 = d > 1 - 1e-5)
LOG_CASES = {
    "sigma_large_rotation_large": ([0.3, -0.2, 0.5, 1.0, -2.0, 0.5, 0.3], 0),
    "sigma_small_rotation_large": ([0.3, -0.2, 0.5, 1.0, -2.0, 0.5, 2e-6], 1),
    "sigma_large_rotation_small": ([1e-3, -2e-3, 5e-4, 1.0, -2.0, 0.5, -0.4], 2),
    "sigma_small_rotation_small": ([1e-3, -2e-3, 5e-4, 1.0, -2.0, 0.5, 2e-6], 3),
    "pure_scale": ([0, 0, 0, 0, 0, 0, 0.7], 2),
}


@pytest.mark.parametrize("name", sorted(LOG_CASES))
def test_log_of_exp_is_the_argument_in_every_branch(name):
    """log(exp(u)) == u.  Tolerance: the chain is about forty operations on numbers of size <= 4 (a few ulp each, 1e-14 in all), except
    that below the d-threshold omega comes from deltaR / 2 (first order, relative error theta^2 / 6 <= 1e-6 of |omega| <= 2.3e-3), which
    also reaches upsilon through A and B."""
    u, branch = LOG_CASES[name]
    T = S.sim3_exp(u)
    assert S.log_branch(T) == branch
    got = S.sim3_log(T)
    tol = 1e-14 if not branch & 2 or name == "pure_scale" else 1e-8
    assert np.abs(got - np.array(u)).max() <= tol, (got, u)


def test_log_of_the_identity_is_zero():
    assert S.log_branch(S.IDENTITY) == 3
    assert np.array_equal(S.sim3_log(S.IDENTITY), np.zeros(7))
    assert np.array_equal(S.sim3_exp(np.zeros(7)), S.IDENTITY)


def test_pure_scale_log():
    T = np.array([0, 0, 0, 1, 0, 0, 0, 2.0])
    assert np.allclose(S.sim3_log(T), [0, 0, 0, 0, 0, 0, np.log(2.0)], rtol=0, atol=1e-16)


@pytest.mark.parametrize("fix_scale", [True, False])
def test_two_vertex_graph_has_the_closed_form_answer(fix_scale):
    """One edge, vertex 0 fixed: the error log(S10 * S0 * S1^-1) vanishes exactly at S1 = S10 * S0, whatever the start.
    Tolerance: the error is evaluated to about 1e-15 and the Jacobian there is well conditioned (the bound of estimate_bounds)."""
    g = S.solve_graph("two", fix_scale)
    r = S.ref_optimize(g)
    want = S.compose(g["meas"][0], g["sim3"][0])
    _, to_truth = S.estimate_bounds(g, r["sim3"])
    assert S.distance(r["sim3"][1:], want[None]) <= to_truth
    assert np.array_equal(r["sim3"][0], g["sim3"][0])


@pytest.mark.parametrize("fix_scale", [True, False])
def test_drifted_ring_returns_to_truth(fix_scale):
    """12 keyframes on a ring, measurements from the true relative poses, initial estimates with accumulated drift.  The residual
    vanishes at truth and Gauss-Newton converges quadratically from a drift of 0.02 per step, so twenty iterations end at the evaluation
    noise: final chi2 <= 1e-12 * initial chi2 (measured: 1e-23 of it), every vertex at truth within estimate_bounds' figure."""
    g = S.make_graph(12, S.ring(12), 21, fix_scale)
    chi0 = S.ref_chi2(g, g["sim3"])
    r = S.ref_optimize(g)
    _, to_truth = S.estimate_bounds(g, r["sim3"])
    print("ring12 fix_scale=%d chi2 %.3e -> %.3e, distance to truth %.3e (bound %.3e), trials %s"
          % (fix_scale, chi0, r["log_chi2"][-1], S.distance(r["sim3"], g["truth"]), to_truth, r["log_trials"].tolist()))
    assert chi0 > 1e-3 and r["log_chi2"][-1] <= 1e-12 * chi0
    assert S.distance(r["sim3"], g["truth"]) <= to_truth
    assert S.ref_chi2(g, r["sim3"]) == r["log_chi2"][-1]


def test_restatement_rejects_trials_from_a_far_start():
    g = S.far_start_graph()
    r = S.ref_optimize(g, **S.FAR)
    print("far start: trials %s, chi2 %.3e -> %s" % (r["log_trials"].tolist(), S.ref_chi2(g, g["sim3"]), r["log_chi2"].tolist()))
    assert 1 < r["log_trials"][0] < 10 and r["n_iterations"] == 3
    assert r["log_chi2"][0] < S.ref_chi2(g, g["sim3"])


def test_branch_graph_covers_every_log_branch_and_fixed_end():
    g = S.branch_graph()
    assert {S.log_branch(T) for T in S.edge_error_transforms(g)} == {0, 1, 2, 3}
    fx = g["fixed"]
    ends = {(int(fx[i]), int(fx[j])) for i, j in g["edges"]}
    assert ends == {(1, 1), (1, 0), (0, 1), (0, 0)}
    lin = S.ref_linearize(g)
    assert not lin["J0"][0].any() and not lin["J1"][0].any() and not lin["J0"][1].any() and lin["J1"][1].any() and not lin["J1"][2].any()


def test_sensitivity_figures():
    """g_e and g_J (essgraph_support.sensitivity) and the per-graph bounds on the final estimates that the GPU tests use; the figures are
    printed for DESIGN.md section 6i.  g_J must be the quotient's amplification of g_e: between g_e / 2e-9 / 100 and 2 * g_e / 2e-9."""
    ge, gj = S.sensitivity()
    print("g_e = %.3e  g_J = %.3e" % (ge, gj))
    assert 0 < ge < 1e-12
    assert ge / 2e-9 / 100 < gj <= 2 * ge / 2e-9
    for shape in S.SOLVE_SHAPES:
        for fix in (True, False):
            g = S.solve_graph(shape, fix)
            r = S.ref_optimize(g)
            between, to_truth = S.estimate_bounds(g, r["sim3"])
            print("%-7s fix_scale=%d  edges %3d  bound between implementations %.3e  bound to truth %.3e  (restatement: %.3e)"
                  % (shape, fix, len(g["edges"]), between, to_truth, S.distance(r["sim3"], g["truth"])))
            assert S.distance(r["sim3"], g["truth"]) <= to_truth


def test_optimizer_adapter_typechecks():
    H = os.path.join(ROOT, "tests", "cpu_harness")
    subprocess.check_call(["g++", "-std=c++14", "-fsyntax-only", "-I" + os.path.join(H, "mock"), "-I" + os.path.join(H, "mockrt"),
                           os.path.join(H, "essgraph_syntax_check.cpp")])


def test_abi_rejects_bad_arguments_without_a_gpu():
    """Every argument check runs before any device work, so this runs anywhere."""
    import ydorbslam_amd as y
    from ydorbslam_amd._lib import YdBaResult
    from ydorbslam_amd.essential_graph import EssentialGraph
    y.build_library()
    L = y.lib()
    g = S.solve_graph("six", True)
    res = YdBaResult()

    def rc(G, out=None):
        return L.ydorb_essential_graph_optimize(C.byref(G.struct), out, C.byref(res))

    def graph(**kw):
        d = dict(sim3=g["sim3"], fixed=g["fixed"], edges=g["edges"], meas=g["meas"])
        d.update(kw)
        return EssentialGraph(**d)

    def rejected(text, code=-1, out=None, **kw):
        assert rc(graph(**kw), out) == code and text in L.ydorb_last_error(), L.ydorb_last_error()

    assert L.ydorb_essential_graph_optimize(None, None, C.byref(res)) == -1
    assert L.ydorb_essential_graph_optimize(C.byref(graph().struct), None, None) == -1
    for field in ("sim3", "fixed", "edge_v0", "edge_v1", "edge_meas"):
        G = graph()
        setattr(G.struct, field, None)
        assert rc(G) == -1 and b"null array" in L.ydorb_last_error()
    pts = np.zeros((3, 3), np.float32)
    G = graph(points=pts, point_ref=[0, 1, 2])
    assert rc(G) == -1 and b"points_out" in L.ydorb_last_error()
    G.struct.point_ref = None
    assert rc(G, pts.ctypes.data_as(C.c_void_p)) == -1 and b"null array" in L.ydorb_last_error()
    rejected(b"point 1 references", points=pts, point_ref=[0, 6, 2], out=pts.ctypes.data_as(C.c_void_p))
    for bad in (-1, 6):
        e = g["edges"].copy()
        e[2, 1] = bad
        rejected(b"edge 2 references", edges=e)
    e = g["edges"].copy()
    e[3] = (4, 4)
    rejected(b"to itself", edges=e)
    rejected(b"no fixed vertex", fixed=np.zeros(6, np.uint8))
    rejected(b"every vertex is fixed", fixed=np.ones(6, np.uint8))
    rejected(b"iterations", iterations=0)
    rejected(b"iterations", max_trials=0)
    rejected(b"lambda_init", lambda_init=0.0)
    s = g["sim3"].copy()
    s[4, 7] = 0.0
    rejected(b"vertex 4 has a non-positive scale", sim3=s)
    m = g["meas"].copy()
    m[1, 7] = -1.0
    rejected(b"edge 1 has a non-positive scale", meas=m)
    G = graph()
    G.struct.device = 16
    assert rc(G) == -1
    # the size limit: the dense solve's rows / 7, named in the text
    n = 2744
    big = EssentialGraph(np.tile(S.IDENTITY, (n, 1)), np.arange(n) == 0, [(i, i + 1) for i in range(n - 1)], np.tile(S.IDENTITY, (n - 1, 1)))
    assert rc(big) == -5 and b"at most 2742" in L.ydorb_last_error()
    assert L.ydorb_essential_graph_release(-1) == -1 and L.ydorb_essential_graph_set_profiling(16, 1) == -1
    assert L.ydorb_essential_graph_linearize(None, None, None, None, None) == -1
