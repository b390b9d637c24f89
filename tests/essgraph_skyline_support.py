"""Test support of the essential graph's block-skyline solver: builds the skyline restatement
tests/essgraph_ref/essgraph_skyline_ref.cpp the way essgraph_support builds the dense one, and names the graphs at which each part of
the plan and of the kernels can go wrong."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

import essgraph_support as S
from essgraph_support import ROOT, _VP, _d, _p

SRC = os.path.join(ROOT, "tests", "essgraph_ref", "essgraph_skyline_ref.cpp")
_REF = None


def sky_ref():
    global _REF
    if _REF is None:
        out = os.path.join(tempfile.mkdtemp(prefix="essskyref"), "libessskyref.so")
        subprocess.check_call(["g++", *S._flags(), "-shared", "-o", out, SRC, "-lm"])
        L = C.CDLL(out)
        L.essref_sky_optimize.restype = C.c_int
        L.essref_sky_optimize.argtypes = [C.c_int, _VP, _VP, C.c_int, _VP, _VP, _VP, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int] + [_VP] * 9
        _REF = L
    return _REF


def sky_ref_optimize(g, points=None, point_ref=None, iterations=20, max_trials=10, lambda_init=1e-16):
    """essgraph_support.ref_optimize on the skyline restatement; the dict also holds skyline_doubles, the entries it stored for H."""
    est = _d(g["sim3"], (-1, 8)).copy()
    v0, v1 = np.ascontiguousarray(g["edges"][:, 0]), np.ascontiguousarray(g["edges"][:, 1])
    pts = np.ascontiguousarray(np.asarray(points if points is not None else np.zeros((0, 3)), np.float32).reshape(-1, 3))
    pref = np.ascontiguousarray(np.asarray(point_ref if point_ref is not None else np.zeros(0), np.int32).reshape(-1))
    P = len(pts)
    out, outd = np.zeros((max(P, 1), 3), np.float32), np.zeros((max(P, 1), 3))
    chi, lam, tr, cnt, sizes = np.zeros(32), np.zeros(32), np.zeros(32, np.int32), np.zeros(3, np.int32), np.zeros(1, np.int64)
    rc = sky_ref().essref_sky_optimize(len(est), _p(est), _p(g["fixed"]), len(v0), _p(v0), _p(v1), _p(_d(g["meas"], (-1, 8))), int(g["fix_scale"]),
                                       iterations, max_trials, lambda_init, P, _p(pts), _p(pref), _p(out), _p(outd), _p(chi), _p(lam), _p(tr), _p(cnt),
                                       _p(sizes))
    assert rc == 0
    n = int(cnt[2])
    return dict(sim3=est, points=out[:P], points_d=outd[:P], n_trials=int(cnt[0]), n_iterations=int(cnt[1]), log_chi2=chi[:n], log_lambda=lam[:n],
                log_trials=tr[:n], skyline_doubles=int(sizes[0]))


def chord_ring_edges(n):
    """tools/essential_graph_bench.py's graph: the loop connection, the spanning chain, chords to i - 2 and, every third keyframe, i - 5"""
    return [(n - 1, 0)] + [(i, i - 1) for i in range(1, n)] + [(i, i - 2) for i in range(2, n)] + [(i, i - 5) for i in range(5, n, 3)]


# What each shape exercises (the solve graphs of essgraph_support come on top):
#   chain3        three free vertices in a row
#   ring12free    the ring closes among free vertices (the fixed one hangs off vertex 5): a full last row in natural order, RCM interleaves
#                 the two arcs, so blocks are stored from the other endpoint's side; the pair (3, 4) is repeated in both directions
#   star_first    hub = the first free vertex: every row starts at column 0, the envelope is dense
#   star_last     hub = the last free vertex: one full row
#   components    two free components off one fixed vertex: a row of length 1 in mid-matrix
#   fixed_only    vertex 5 has fixed neighbours only: a 1-block row and an empty column list
#   ring300       300 keyframes, chords to i - 2 and every third i - 5, vertex 0 fixed, so a plain band: rows of at most 6 blocks and
#                 column lists of at most 4 rows, but more block columns than a workgroup has waves or threads
#   ring300free   the same ring closed among free vertices (the fixed vertex 300 hangs off vertex 5): in natural order the last row has 300
#                 blocks, 2 093 items of the back substitution, nine passes of the 256 threads; every column list holds that row
#   star60_first  hub = the first of 60 free vertices: a dense envelope.  Column 0 lists 59 rows, 414 panel rows with b (two passes of the
#                 256 threads), the rows grow to 60 blocks (413 items of the back substitution), 86 730 update items at column 0
#   star60_last   hub = the last of 60 free vertices: one row of 60 blocks over 59 columns whose lists hold that row alone
# The two star60 shapes and ring300free are the ones that enter k_ess_sky_solve's loops past a thread's first item in the panel and in
# the back substitution; the update's loop is entered from tree40 on.
EXTRA_SHAPES = ["chain3", "ring12free", "star_first", "star_last", "components", "fixed_only", "ring300", "ring300free", "star60_first", "star60_last"]
WIDE_SHAPES = ["ring300free", "star60_first", "star60_last"]
TRIAL_SHAPES = ["two", "ring12", "tree40"] + EXTRA_SHAPES


@functools.lru_cache(maxsize=None)
def shape_graph(shape, fix_scale):
    if shape in S.SOLVE_SHAPES:
        return S.solve_graph(shape, fix_scale)
    seed = 100 + 2 * EXTRA_SHAPES.index(shape) + int(fix_scale)
    if shape == "chain3":
        return S.make_graph(4, [(0, 1), (1, 2), (2, 3)], seed, fix_scale, name=shape)
    if shape == "ring12free":
        return S.make_graph(13, S.ring(12, repeated=[(3, 4), (4, 3)]) + [(12, 5)], seed, fix_scale, fixed=(12,), name=shape)
    if shape == "star_first":
        return S.make_graph(9, [(0, 1)] + [(1, v) for v in range(2, 9)], seed, fix_scale, name=shape)
    if shape == "star_last":
        return S.make_graph(9, [(0, 8)] + [(v, 8) for v in range(1, 8)], seed, fix_scale, name=shape)
    if shape == "components":
        return S.make_graph(8, [(0, 1), (1, 2), (2, 3), (3, 1), (0, 4), (4, 5), (5, 6), (6, 7), (7, 4)], seed, fix_scale, name=shape)
    if shape == "fixed_only":
        return S.make_graph(8, [(0, 1), (1, 2), (2, 3), (3, 4), (0, 5), (5, 3), (3, 6), (6, 7), (7, 4)], seed, fix_scale, drift=0.01, fixed=(0, 3),
                            name=shape)
    if shape == "ring300":
        return S.make_graph(300, chord_ring_edges(300), seed, fix_scale, drift=0.002, name=shape)
    if shape == "ring300free":
        return S.make_graph(301, chord_ring_edges(300) + [(300, 5)], seed, fix_scale, drift=0.002, fixed=(300,), name=shape)
    if shape == "star60_first":
        return S.make_graph(61, [(0, 1)] + [(1, v) for v in range(2, 61)], seed, fix_scale, drift=0.01, name=shape)
    if shape == "star60_last":
        return S.make_graph(61, [(0, 60)] + [(v, 60) for v in range(1, 60)], seed, fix_scale, drift=0.01, name=shape)
    raise KeyError(shape)


def plain_graph(n, edges, fixed=(0,)):
    """A graph for the host-only plan: identity poses and measurements, which the plan never reads"""
    mask = np.zeros(n, np.uint8)
    mask[list(fixed)] = 1
    edges = np.asarray(edges, np.int32).reshape(-1, 2)
    return dict(n=n, sim3=np.tile(S.IDENTITY, (n, 1)), fixed=mask, edges=edges, meas=np.tile(S.IDENTITY, (len(edges), 1)), fix_scale=True)


def check_plan(g, p):
    """The properties of a plan dict (ydorbslam_amd.essential_graph.plan) on graph g"""
    free = np.nonzero(g["fixed"] == 0)[0]
    nf = len(free)
    free_of = {int(v): k for k, v in enumerate(free)}
    perm, first = p["perm"], p["first"]
    assert p["n_free"] == nf and sorted(perm.tolist()) == list(range(nf))
    inv = np.empty(nf, np.int64)
    inv[perm] = np.arange(nf)
    assert (first <= np.arange(nf)).all() and (first >= 0).all()
    lowest = np.arange(nf)
    for i, j in g["edges"]:
        if int(i) in free_of and int(j) in free_of:
            a, b = inv[free_of[int(i)]], inv[free_of[int(j)]]
            assert first[max(a, b)] <= min(a, b)
            lowest[max(a, b)] = min(lowest[max(a, b)], min(a, b))
    assert np.array_equal(first, lowest)
    assert p["envelope_blocks"] == int((np.arange(nf) - first + 1).sum()) and p["max_row_blocks"] == int((np.arange(nf) - first + 1).max())
    assert p["envelope_blocks"] == (p["envelope_blocks_rcm"] if p["ordering_used"] == "rcm" else p["envelope_blocks_natural"])
