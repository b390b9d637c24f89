"""Essential-graph optimisation of loop closing (Optimizer::optimizeEssentialGraph) on the GPU through the C ABI
(include/ydorb/c_api.h, "Essential-graph optimisation").  Restates ORB-SLAM2's Optimizer::OptimizeEssentialGraph, which YDORBSLAM
renames; DESIGN.md section 6i has the contract, the limits and the timings, section 6j the block-skyline solver that
solver="skyline" (or "auto" above the dense solver's 2 742 free keyframes) selects."""
import ctypes as C

import numpy as np

from ._lib import YdBaResult, YdEssentialGraph, YdEssentialSolverInfo, YdEssentialSolverOptions, check, lib

SOLVERS = {"auto": 0, "dense": 1, "skyline": 2}
ORDERINGS = {"smaller": 0, "natural": 1, "rcm": 2}


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


def _options(solver, ordering, max_factor_bytes):
    """None when no argument was given: the call then goes through the entry without options (the dense solver)."""
    if solver is None and ordering is None and max_factor_bytes is None:
        return None
    num = lambda v, names: names[v] if isinstance(v, str) else int(v or 0)
    return YdEssentialSolverOptions(num(solver, SOLVERS), num(ordering, ORDERINGS), int(max_factor_bytes or 0))


def _info(info):
    names = lambda table, v: next(k for k, n in table.items() if n == v)
    return dict(solver_used=names(SOLVERS, info.solver_used), ordering_used=names(ORDERINGS, info.ordering_used), n_free=info.n_free,
                max_row_blocks=info.max_row_blocks, envelope_blocks=info.envelope_blocks, envelope_blocks_natural=info.envelope_blocks_natural,
                envelope_blocks_rcm=info.envelope_blocks_rcm, factor_bytes=info.factor_bytes)


def plan(sim3, fixed, edges, meas, fix_scale=True, solver="auto", ordering="smaller", max_factor_bytes=0, device=0):
    """ydorb_essential_graph_plan, on the host alone: dict(info..., perm [free vertices] = the free vertex at each position of the
    factor, first [free vertices] = the first column of each row's envelope, by position)."""
    G = EssentialGraph(sim3, fixed, edges, meas, fix_scale=fix_scale, device=device)
    nf = int((G.fixed == 0).sum())
    perm, first = np.zeros(max(nf, 1), np.int32), np.zeros(max(nf, 1), np.int32)
    info = YdEssentialSolverInfo()
    opt = _options(solver, ordering, max_factor_bytes)
    check(lib().ydorb_essential_graph_plan(C.byref(G.struct), C.byref(opt), C.byref(info), _p(perm), _p(first)))
    r = _info(info)
    r.update(perm=perm[:nf], first=first[:nf])
    return r


def _log(res):
    n = res.n_log
    return dict(n_trials=res.n_trials, n_iterations=res.n_iterations, log_chi2=np.array(res.log_chi2[:n]), log_lambda=np.array(res.log_lambda[:n]),
                log_trials=np.array(res.log_trials[:n], np.int32),
                ms=dict(linearize=res.ms_build, assemble=res.ms_schur, solve=res.ms_solve, update=res.ms_update, chi2=res.ms_errors))


def optimize_essential_graph(sim3, fixed, edges, meas, points=None, point_ref=None, fix_scale=True, iterations=20, max_trials=10,
                             lambda_init=1e-16, device=0, solver=None, ordering=None, max_factor_bytes=None):
    """One ydorb_essential_graph_optimize call, or, when solver ("auto", "dense", "skyline"), ordering ("smaller", "natural", "rcm") or
    max_factor_bytes is given, one ydorb_essential_graph_optimize_with call.  Returns dict(sim3 [V,8] optimised, points [P,3] float32
    corrected, n_trials, n_iterations, log_chi2, log_lambda, log_trials, ms) and, through the second entry, info (see plan)."""
    G = EssentialGraph(sim3, fixed, edges, meas, points, point_ref, fix_scale, iterations, max_trials, lambda_init, device)
    out = np.zeros((max(len(G.points), 1), 3), np.float32)
    res = YdBaResult()
    opt = _options(solver, ordering, max_factor_bytes)
    if opt is None:
        check(lib().ydorb_essential_graph_optimize(C.byref(G.struct), _p(out), C.byref(res)))
        r = _log(res)
    else:
        info = YdEssentialSolverInfo()
        check(lib().ydorb_essential_graph_optimize_with(C.byref(G.struct), C.byref(opt), _p(out), C.byref(res), C.byref(info)))
        r = _log(res)
        r["info"] = _info(info)
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


def trial_step(sim3, fixed, edges, meas, lam, fix_scale=True, device=0, solver=None, ordering=None, max_factor_bytes=None, return_system=False):
    """Test / debug: the update x [free vertices, 7] one LM trial with lambda = lam solves for at the estimate handed in, and whether the
    factorisation reported a solve.  solver / ordering / max_factor_bytes as in optimize_essential_graph (ydorb_essential_graph_
    trial_step_with, which takes any lambda).  return_system: also H [7F,7F] (without lambda) and b [7F] as assembled, in vertex order."""
    G = EssentialGraph(sim3, fixed, edges, meas, fix_scale=fix_scale, device=device)
    nf = int((G.fixed == 0).sum())
    x = np.full((nf, 7), np.nan)
    solved = C.c_int32(-1)
    opt = _options(solver, ordering, max_factor_bytes)
    if opt is None and not return_system:
        check(lib().ydorb_essential_graph_trial_step(C.byref(G.struct), float(lam), _p(x), C.byref(solved)))
        return x, bool(solved.value)
    opt = opt or YdEssentialSolverOptions(SOLVERS["dense"], 0, 0)
    H, b = (np.full((7 * nf, 7 * nf), np.nan), np.full(7 * nf, np.nan)) if return_system else (None, None)
    check(lib().ydorb_essential_graph_trial_step_with(C.byref(G.struct), C.byref(opt), float(lam), _p(x), C.byref(solved), _p(H), _p(b)))
    return (x, bool(solved.value), H, b) if return_system else (x, bool(solved.value))


def set_profiling(on, device=0):
    """ydorb_essential_graph_set_profiling: fill the ms fields of later calls from HIP event pairs."""
    check(lib().ydorb_essential_graph_set_profiling(device, int(bool(on))))


def release(device=0):
    """ydorb_essential_graph_release: give the scratch of `device` back."""
    check(lib().ydorb_essential_graph_release(device))
