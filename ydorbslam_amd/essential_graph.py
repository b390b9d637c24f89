"""Essential-graph optimisation of loop closing (Optimizer::optimizeEssentialGraph) on the GPU through the C ABI
(include/ydorb/c_api.h, "Essential-graph optimisation").  Restates ORB-SLAM2's Optimizer::OptimizeEssentialGraph, which YDORBSLAM
renames; DESIGN.md section 6i has the contract, the limits and the timings."""
import ctypes as C

import numpy as np

from ._lib import YdBaResult, YdEssentialGraph, check, lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class EssentialGraph:
    """The flat arrays of one call, kept alive next to the C struct.  sim3 [V,8] = qx qy qz qw tx ty tz s (Scw), fixed [V],
    edges [E,2] = (vertex(0) = i, vertex(1) = j), meas [E,8] = Sji, points [P,3] float32 with point_ref [P]."""

    def __init__(self, sim3, fixed, edges, meas, points=None, point_ref=None, fix_scale=True, iterations=20, max_trials=10,
                 lambda_init=1e-16, device=0):
        self.sim3 = np.ascontiguousarray(np.array(sim3, np.float64).reshape(-1, 8))
        self.fixed = np.ascontiguousarray(np.asarray(fixed).astype(np.uint8).reshape(-1))
        edges = np.asarray(edges, np.int32).reshape(-1, 2)
        self.v0 = np.ascontiguousarray(edges[:, 0])
        self.v1 = np.ascontiguousarray(edges[:, 1])
        self.meas = np.ascontiguousarray(np.asarray(meas, np.float64).reshape(-1, 8))
        self.points = np.ascontiguousarray(np.asarray(points if points is not None else np.zeros((0, 3)), np.float32).reshape(-1, 3))
        self.point_ref = np.ascontiguousarray(np.asarray(point_ref if point_ref is not None else np.zeros(0), np.int32).reshape(-1))
        assert len(self.fixed) == len(self.sim3) and len(self.meas) == len(self.v0) and len(self.point_ref) == len(self.points)
        nz = lambda a: _p(a) if a.size else None
        self.struct = YdEssentialGraph(device, len(self.sim3), len(self.v0), len(self.points), _p(self.sim3), _p(self.fixed), nz(self.v0), nz(self.v1),
                                       nz(self.meas), nz(self.points), nz(self.point_ref), int(bool(fix_scale)), int(iterations), int(max_trials),
                                       float(lambda_init))


def _log(res):
    n = res.n_log
    return dict(n_trials=res.n_trials, n_iterations=res.n_iterations, log_chi2=np.array(res.log_chi2[:n]), log_lambda=np.array(res.log_lambda[:n]),
                log_trials=np.array(res.log_trials[:n], np.int32),
                ms=dict(linearize=res.ms_build, assemble=res.ms_schur, solve=res.ms_solve, update=res.ms_update, chi2=res.ms_errors))


def optimize_essential_graph(sim3, fixed, edges, meas, points=None, point_ref=None, fix_scale=True, iterations=20, max_trials=10,
                             lambda_init=1e-16, device=0):
    """One ydorb_essential_graph_optimize call.  Returns dict(sim3 [V,8] optimised, points [P,3] float32 corrected, n_trials,
    n_iterations, log_chi2, log_lambda, log_trials, ms)."""
    G = EssentialGraph(sim3, fixed, edges, meas, points, point_ref, fix_scale, iterations, max_trials, lambda_init, device)
    out = np.zeros((max(len(G.points), 1), 3), np.float32)
    res = YdBaResult()
    check(lib().ydorb_essential_graph_optimize(C.byref(G.struct), _p(out), C.byref(res)))
    r = _log(res)
    r.update(sim3=G.sim3, points=out[:len(G.points)])
    return r


def linearize_essential_graph(sim3, fixed, edges, meas, fix_scale=True, device=0):
    """Test / debug: what k_ess_linearize stores at the estimate handed in: dict(err [E,7], J0, J1 [E,7,7], chi2 [E])."""
    G = EssentialGraph(sim3, fixed, edges, meas, fix_scale=fix_scale, device=device)
    E = max(len(G.v0), 1)
    err, J0, J1, chi = np.zeros((E, 7)), np.zeros((E, 7, 7)), np.zeros((E, 7, 7)), np.zeros(E)
    check(lib().ydorb_essential_graph_linearize(C.byref(G.struct), _p(err), _p(J0), _p(J1), _p(chi)))
    E = len(G.v0)
    return dict(err=err[:E], J0=J0[:E], J1=J1[:E], chi2=chi[:E])


def trial_step(sim3, fixed, edges, meas, lam, fix_scale=True, device=0):
    """Test / debug: the update x [free vertices, 7] one LM trial with lambda = lam solves for at the estimate handed in, and whether the
    factorisation reported a solve."""
    G = EssentialGraph(sim3, fixed, edges, meas, fix_scale=fix_scale, device=device)
    x = np.full((int((G.fixed == 0).sum()), 7), np.nan)
    solved = C.c_int32(-1)
    check(lib().ydorb_essential_graph_trial_step(C.byref(G.struct), float(lam), _p(x), C.byref(solved)))
    return x, bool(solved.value)


def set_profiling(on, device=0):
    """ydorb_essential_graph_set_profiling: fill the ms fields of later calls from HIP event pairs."""
    check(lib().ydorb_essential_graph_set_profiling(device, int(bool(on))))


def release(device=0):
    """ydorb_essential_graph_release: give the scratch of `device` back."""
    check(lib().ydorb_essential_graph_release(device))
