"""Test support of the essential-graph optimisation: builds the CPU restatement tests/essgraph_ref/essgraph_ref.cpp with
oracle/Makefile's compiler flags, makes pose graphs with a known answer, and derives the tolerances of the GPU tests from the
restatement's own sensitivity."""
import ctypes as C
import functools
import os
import re
import shlex
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "essgraph_ref", "essgraph_ref.cpp")
_REF = None
_VP = C.c_void_p


def _flags():
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return shlex.split(re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1))


def ref():
    global _REF
    if _REF is None:
        out = os.path.join(tempfile.mkdtemp(prefix="essref"), "libessref.so")
        subprocess.check_call(["g++", *_flags(), "-shared", "-o", out, SRC, "-lm"])
        L = C.CDLL(out)
        L.essref_log_branch.restype = C.c_int
        L.essref_optimize.restype = C.c_int
        L.essref_optimize.argtypes = [C.c_int, _VP, _VP, C.c_int, _VP, _VP, _VP, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int] + [_VP] * 8
        L.essref_linearize.argtypes = [C.c_int, _VP, _VP, C.c_int, _VP, _VP, _VP, C.c_int, C.c_int] + [_VP] * 4
        L.essref_chi2.restype = C.c_double
        L.essref_chi2.argtypes = [C.c_int, _VP, C.c_int, _VP, _VP, _VP]
        _REF = L
    return _REF


def _p(a):
    return a.ctypes.data_as(_VP)


def _d(a, n):
    return np.ascontiguousarray(np.asarray(a, np.float64).reshape(n))


# ------------------------------------------------------------------------------------------------------------ Sim3 on the restatement
def sim3_exp(u):
    out = np.zeros(8)
    ref().essref_exp(_p(_d(u, 7)), _p(out))
    return out


def sim3_log(S):
    out = np.zeros(7)
    ref().essref_log(_p(_d(S, 8)), _p(out))
    return out


def log_branch(S):
    """bit 0: |sigma| < 1e-5, bit 1: d > 1 - 1e-5"""
    return ref().essref_log_branch(_p(_d(S, 8)))


def compose(a, b):
    out = np.zeros(8)
    ref().essref_compose(_p(_d(a, 8)), _p(_d(b, 8)), _p(out))
    return out


def inverse(a):
    out = np.zeros(8)
    ref().essref_inverse(_p(_d(a, 8)), _p(out))
    return out


IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0, 1.0])


def distance(A, B):
    """max over vertices of |log(A_v * B_v^-1)|_2"""
    A, B = np.asarray(A).reshape(-1, 8), np.asarray(B).reshape(-1, 8)
    return max(float(np.linalg.norm(sim3_log(compose(a, inverse(b))))) for a, b in zip(A, B))


# ------------------------------------------------------------------------------------------------------------ graphs with a known answer
def make_graph(n, edges, seed, fix_scale, drift=0.02, fixed=(0,), name=""):
    """n keyframes on a loop of radius 5 looking around (Scw, scale 1 under fix_scale, else 0.8..1.25), every measurement the true
    relative pose Sji = Sjw * Swi, the initial estimates the truth with a drift that accumulates from the first fixed vertex on
    (a random 7-vector of size `drift` per step, without scale under fix_scale).  Truth is the unique minimum (chi2 = 0): the fixed
    vertices are left at it."""
    rng = np.random.default_rng(seed)
    truth = np.zeros((n, 8))
    for v in range(n):
        a = 2 * np.pi * v / max(n, 8)
        u = np.concatenate([[0.1 * np.sin(3 * a), a, 0.1 * np.cos(2 * a)], 5 * np.array([np.cos(a), 0.1 * np.sin(5 * a), np.sin(a)]),
                            [0.0 if fix_scale else rng.uniform(np.log(0.8), np.log(1.25))]])
        truth[v] = sim3_exp(u)
    fixed_mask = np.zeros(n, np.uint8)
    fixed_mask[list(fixed)] = 1
    est = truth.copy()
    D = IDENTITY
    for v in range(n):
        if fixed_mask[v]:
            continue
        step = rng.normal(0, drift, 7)
        if fix_scale:
            step[6] = 0
        D = compose(sim3_exp(step), D)
        est[v] = compose(D, truth[v])
    edges = np.asarray(edges, np.int32).reshape(-1, 2)
    meas = np.stack([compose(truth[j], inverse(truth[i])) for i, j in edges])
    return dict(name=name, n=n, sim3=est, truth=truth, fixed=fixed_mask, edges=edges, meas=meas, fix_scale=bool(fix_scale))


def ring(n, chords=(), repeated=()):
    e = [(i, i + 1) for i in range(n - 1)] + [(n - 1, 0)]
    return e + list(chords) + list(repeated)


def tree40():
    """40 vertices: a spanning tree (parent = (v - 1) // 2 ... a binary heap turned into child -> parent edges as the reference adds
    them), covisibility chords between siblings and two loop connections."""
    tree = [(v, (v - 1) // 2) for v in range(1, 40)]
    chords = [(v, v + 1) for v in range(1, 39, 2)] + [(v, v + 5) for v in range(3, 30, 7)]
    loops = [(39, 0), (31, 16)]
    return loops + tree + chords


SOLVE_SHAPES = ["two", "six", "v33", "ring12", "tree40"]


@functools.lru_cache(maxsize=None)
def solve_graph(shape, fix_scale):
    """The shapes of the whole-solve tests.  six: 35 rows, padded to 64 (the pad crosses a tile); v33: 224 rows = 7 full tiles, no pad;
    ring12 repeats the pair (3, 4) in both directions; tree40: spanning tree, chords, two loop connections."""
    seed = {"two": 1, "six": 2, "v33": 3, "ring12": 4, "tree40": 5}[shape] * 2 + int(fix_scale)
    if shape == "two":
        return make_graph(2, [(0, 1)], seed, fix_scale, drift=0.05, name=shape)
    if shape == "six":
        return make_graph(6, ring(6, chords=[(1, 4)]), seed, fix_scale, name=shape)
    if shape == "v33":
        return make_graph(33, ring(33, chords=[(2, 20), (7, 28), (11, 12)]), seed, fix_scale, drift=0.01, name=shape)
    if shape == "ring12":
        return make_graph(12, ring(12, repeated=[(3, 4), (4, 3)]), seed, fix_scale, name=shape)
    if shape == "tree40":
        return make_graph(40, tree40(), seed, fix_scale, drift=0.01, name=shape)
    raise KeyError(shape)


FAR = dict(iterations=3, lambda_init=1e-16)


def far_start_graph():
    """A ring with free scale whose drift (1.2 per step) puts the start far outside the basin of truth.  The first Gauss-Newton step
    raises chi2 above the start's 5441 (so the decision is nowhere near the evaluation noise) and is rejected; with lambda at 1e-16
    the next trials repeat it, until lambda has doubled, quadrupled, ... its way to a size that damps the step."""
    return make_graph(10, ring(10, chords=[(2, 7)]), 34, False, drift=1.2)


@functools.lru_cache(maxsize=None)
def branch_graph():
    """Eight edges over six vertices (0 and 1 fixed, scale free) whose errors take each branch of Sim3::log.  The estimate of a vertex
    is P * truth with a chosen P, so an edge (i, j) with P_i = I has the error P_j^-1 and one with P_j = I a conjugate of P_i (same
    angle, same scale).  Vertices 0, 2, 4 sit at truth, 1 has a full perturbation, 3 a rotation (sigma = 0), 5 a scale (omega = 0).
      (0, 1) both ends fixed, rotation and scale    (0, 2) fixed at vertex(0), identity error: |sigma| < eps, d > 1 - eps
      (3, 0) fixed at vertex(1), rotation only      (2, 3), (3, 4) rotation only: |sigma| < eps, d below
      (4, 5), (2, 5) scale only: d > 1 - eps        (3, 5) rotation and scale among free vertices"""
    g = make_graph(6, [(0, 1), (0, 2), (3, 0), (2, 3), (3, 4), (4, 5), (2, 5), (3, 5)], 11, False, drift=0.0, fixed=(0, 1), name="branches")
    est = g["truth"].copy()
    est[1] = compose(sim3_exp([0.02, -0.01, 0.03, 0.1, 0.0, -0.1, 0.05]), est[1])
    est[3] = compose(sim3_exp([0.3, -0.2, 0.1, 0.05, 0.02, 0.0, 0.0]), est[3])
    est[5] = compose(sim3_exp([0.0, 0.0, 0.0, 0.05, 0.02, -0.03, 0.2]), est[5])
    g["sim3"] = est
    return g


def edge_error_transforms(g):
    return [compose(compose(m, g["sim3"][i]), inverse(g["sim3"][j])) for (i, j), m in zip(g["edges"], g["meas"])]


# ------------------------------------------------------------------------------------------------------------ the restatement
def ref_linearize(g, long_double=False, sim3=None):
    E = len(g["edges"])
    est = _d(g["sim3"] if sim3 is None else sim3, (-1, 8))
    v0, v1 = np.ascontiguousarray(g["edges"][:, 0]), np.ascontiguousarray(g["edges"][:, 1])
    err, J0, J1, chi = np.zeros((E, 7)), np.zeros((E, 7, 7)), np.zeros((E, 7, 7)), np.zeros(E)
    ref().essref_linearize(len(est), _p(est), _p(g["fixed"]), E, _p(v0), _p(v1), _p(_d(g["meas"], (-1, 8))), int(g["fix_scale"]), int(long_double),
                           _p(err), _p(J0), _p(J1), _p(chi))
    return dict(err=err, J0=J0, J1=J1, chi2=chi)


def ref_chi2(g, sim3):
    est = _d(sim3, (-1, 8))
    v0, v1 = np.ascontiguousarray(g["edges"][:, 0]), np.ascontiguousarray(g["edges"][:, 1])
    return ref().essref_chi2(len(est), _p(est), len(v0), _p(v0), _p(v1), _p(_d(g["meas"], (-1, 8))))


def ref_optimize(g, points=None, point_ref=None, iterations=20, max_trials=10, lambda_init=1e-16):
    est = _d(g["sim3"], (-1, 8)).copy()
    v0, v1 = np.ascontiguousarray(g["edges"][:, 0]), np.ascontiguousarray(g["edges"][:, 1])
    pts = np.ascontiguousarray(np.asarray(points if points is not None else np.zeros((0, 3)), np.float32).reshape(-1, 3))
    pref = np.ascontiguousarray(np.asarray(point_ref if point_ref is not None else np.zeros(0), np.int32).reshape(-1))
    P = len(pts)
    out, outd = np.zeros((max(P, 1), 3), np.float32), np.zeros((max(P, 1), 3))
    chi, lam, tr, cnt = np.zeros(32), np.zeros(32), np.zeros(32, np.int32), np.zeros(3, np.int32)
    rc = ref().essref_optimize(len(est), _p(est), _p(g["fixed"]), len(v0), _p(v0), _p(v1), _p(_d(g["meas"], (-1, 8))), int(g["fix_scale"]), iterations,
                               max_trials, lambda_init, P, _p(pts), _p(pref), _p(out), _p(outd), _p(chi), _p(lam), _p(tr), _p(cnt))
    assert rc == 0
    n = int(cnt[2])
    return dict(sim3=est, points=out[:P], points_d=outd[:P], n_trials=int(cnt[0]), n_iterations=int(cnt[1]), log_chi2=chi[:n], log_lambda=lam[:n],
                log_trials=tr[:n])


# ------------------------------------------------------------------------------------------------------------ tolerances
def gpu_test_graphs():
    return [branch_graph()] + [solve_graph(s, f) for s in SOLVE_SHAPES for f in (True, False)]


@functools.lru_cache(maxsize=None)
def sensitivity():
    """(g_e, g_J): the largest gap of the restatement's per-edge error vector and Jacobian entries between the error chain in double and
    in long double (rounded to double before the difference quotient is taken), over the graphs of the GPU tests.  A device acos / log /
    sin / cos that differs from the host's by a few ulp perturbs the chain the same way; the quotient divides it by 2e-9."""
    ge = gj = 0.0
    for g in gpu_test_graphs():
        a, b = ref_linearize(g), ref_linearize(g, long_double=True)
        ge = max(ge, float(np.abs(a["err"] - b["err"]).max()))
        gj = max(gj, float(np.abs(a["J0"] - b["J0"]).max()), float(np.abs(a["J1"] - b["J1"]).max()))
    return ge, gj


MARGIN = 16   # transcendental ulp differences compounding through exp, product and log


def stacked_jacobian(g, sim3):
    """The Jacobian of all residuals with respect to the free vertices' updates at `sim3` (columns that are zero by construction -
    the scale under fix_scale - dropped)."""
    lin = ref_linearize(g, sim3=sim3)
    free = np.nonzero(g["fixed"] == 0)[0]
    col = {int(v): k for k, v in enumerate(free)}
    E = len(g["edges"])
    J = np.zeros((7 * E, 7 * len(free)))
    for e, (i, j) in enumerate(g["edges"]):
        if int(i) in col:
            J[7 * e:7 * e + 7, 7 * col[int(i)]:7 * col[int(i)] + 7] = lin["J0"][e]
        if int(j) in col:
            J[7 * e:7 * e + 7, 7 * col[int(j)]:7 * col[int(j)] + 7] = lin["J1"][e]
    if g["fix_scale"]:
        J = J[:, [c for c in range(J.shape[1]) if c % 7 != 6]]
    return J


def estimate_bounds(g, final):
    """(bound between two implementations, bound against truth) on distance() of the final estimates, from the restatement alone.
    Both run Gauss-Newton steps x = -(J^T J)^-1 J^T e (lambda is 1e-16) on a problem whose residual vanishes at the answer.
      * Two implementations whose Jacobian entries differ by at most MARGIN * g_J: a least-squares solution moves by at most
        2 kappa(J) |dJ|_F / |J|_2 of its own size when J moves by dJ and the residual is small (Golub & Van Loan 5.3.7), and no step
        is larger than the whole correction |x| = |log(final * initial^-1)| stacked over the vertices.  Later steps correct earlier
        ones, so this over-states the final gap; it is the bound that needs no model of the iteration.
      * Against truth: the evaluation noise of the error vector, MARGIN * g_e per entry, is indistinguishable from a residual of that
        size, which moves the minimum by at most |de|_2 / sigma_min(J); the same applies to each implementation, hence the factor 2."""
    ge, gj = sensitivity()
    J = stacked_jacobian(g, final)
    sv = np.linalg.svd(J, compute_uv=False)
    E = len(g["edges"])
    x = np.concatenate([sim3_log(compose(a, inverse(b))) for a, b, f in zip(final, g["sim3"], g["fixed"]) if not f])
    between = 2 * (sv[0] / sv[-1]) * (MARGIN * gj * np.sqrt(98 * E)) / sv[0] * float(np.linalg.norm(x))
    truth = 2 * MARGIN * ge * np.sqrt(7 * E) / sv[-1]
    return float(between), float(truth)


def iterations_above_noise(g, log_chi2):
    """How many leading iterations of a log end at a chi2 that is still far above its own evaluation noise.  With every error entry
    uncertain by de_k <= MARGIN * g_e, chi2 is uncertain by 2 sqrt(chi2) |de| + |de|^2, |de|^2 = 7 E (MARGIN g_e)^2.  An iteration that
    ends at chi2 >= 1e4 |de|^2 knows that chi2 to 2 %, and the chi2 it started from (larger by orders: the convergence is quadratic)
    better still, so its accept / reject decisions do not depend on the noise.  Below that an implementation's own rounding decides."""
    de2 = 7 * len(g["edges"]) * (MARGIN * sensitivity()[0]) ** 2
    above = np.asarray(log_chi2) >= 1e4 * de2
    return int(np.argmin(above)) if not above.all() else len(above)


def map_points(n, n_vertices, seed, always=()):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-6, 6, (n, 3)).astype(np.float32)
    refv = rng.integers(0, n_vertices, n).astype(np.int32)
    for k, v in enumerate(always):
        if k < n:
            refv[k] = v
    return pts, refv
