"""Generators and checks of the BA block-skyline tests (test_ba_skyline_cpu.py, test_ba_skyline_gpu.py, test_gba_skyline_adapter_gpu.py;
DESIGN.md section 6k): trajectory-shaped BA problems, disjoint copies of one problem, a numpy statement of the envelope, block-SPD
systems and the condition-free residual bound of section 6j."""
import os

import numpy as np

from ydorbslam_amd.synth import TRAJECTORY_CLOSURE, trajectory_ba_problem as trajectory_problem   # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAMERA = np.array([500.0, 500.0, 320.0, 240.0, 40.0])      # synth's
CLOSURE = TRAJECTORY_CLOSURE


def graph_problem(K, lists, fixed=(0,)):
    """A problem with the given structure only (for the host plan, which reads no geometry): lists[p] = the keyframes that see point p."""
    ep = np.array([k for l in lists for k in l], np.int32)
    eq = np.array([p for p, l in enumerate(lists) for _ in l], np.int32)
    poses = np.zeros((K, 7))
    poses[:, 6] = 1.0
    fixed_mask = np.zeros(K, np.uint8)
    fixed_mask[list(fixed)] = 1
    return dict(poses=poses, fixed=fixed_mask, points=np.zeros((max(len(lists), 1), 3)), edge_pose=ep, edge_point=eq, meas=np.zeros((len(ep), 3)),
                info=np.ones(len(ep)), camera=CAMERA.copy())


def copies(prob, n):
    """n disjoint copies of prob in one problem: copy c's keyframes, points and edges are prob's, index-shifted; each has its own fixed
    keyframes."""
    K, P = len(prob["poses"]), len(prob["points"])
    out = dict(camera=prob["camera"].copy())
    for key in ("poses", "fixed", "points", "meas", "info"):
        out[key] = np.concatenate([prob[key]] * n)
    out["edge_pose"] = np.concatenate([prob["edge_pose"] + c * K for c in range(n)]).astype(np.int32)
    out["edge_point"] = np.concatenate([prob["edge_point"] + c * P for c in range(n)]).astype(np.int32)
    return out


def free_index(prob):
    """free-pose index of every keyframe (-1: fixed, or without an edge), as the solver numbers them"""
    used = np.zeros(len(prob["fixed"]), bool)
    used[prob["edge_pose"]] = True
    free = used & (np.asarray(prob["fixed"]) == 0)
    idx = np.full(len(free), -1, np.int64)
    idx[free] = np.arange(int(free.sum()))
    return idx


def numpy_pairs(prob):
    """The distinct unordered pairs of free poses that share a point, as a set of (i1, i2), i1 < i2, by numpy and Python sets alone."""
    idx = free_index(prob)
    f = idx[prob["edge_pose"]]
    order = np.argsort(prob["edge_point"], kind="stable")
    pt, f = np.asarray(prob["edge_point"])[order], f[order]
    pairs = set()
    bounds = np.flatnonzero(np.diff(pt)) + 1
    for seg in np.split(f, bounds):
        s = np.unique(seg[seg >= 0])
        for a in range(len(s)):
            for b in range(a + 1, len(s)):
                pairs.add((int(s[a]), int(s[b])))
    return pairs


def numpy_envelope(pairs, perm):
    """first[] by position and the number of envelope blocks under the order perm (perm[k] = free pose at position k)"""
    n = len(perm)
    inv = np.empty(n, np.int64)
    inv[np.asarray(perm)] = np.arange(n)
    first = np.arange(n)
    for a, b in pairs:
        lo, hi = sorted((inv[a], inv[b]))
        first[hi] = min(first[hi], lo)
    return first, int(np.sum(np.arange(n) - first + 1))


def check_plan(prob, plan):
    """perm is a permutation, first[k] <= k, and first / the sizes are the numpy statement's."""
    pairs = numpy_pairs(prob)
    n = plan["n_free"]
    assert n == int((free_index(prob) >= 0).sum())
    assert plan["covisible_pairs"] == len(pairs)
    if n == 0:
        return
    assert sorted(plan["perm"].tolist()) == list(range(n))
    assert (plan["first"] <= np.arange(n)).all() and (plan["first"] >= 0).all()
    first, blocks = numpy_envelope(pairs, plan["perm"])
    assert np.array_equal(first, plan["first"]) and blocks == plan["envelope_blocks"]
    assert plan["max_row_blocks"] == int(np.max(np.arange(n) - first + 1))
    assert plan["envelope_blocks_natural"] == numpy_envelope(pairs, np.arange(n))[1]


# ---- block-SPD systems for the factorisation alone -----------------------------------------------------------------------------------
def block_spd(n_blocks, block_pairs, seed, bad_block=None):
    """A [6 n, 6 n] with a random 6x6 block for every pair in block_pairs (both triangles) and diagonal blocks that make it strictly
    diagonally dominant, so SPD whatever the pattern; b random.  bad_block: that diagonal block is negated (not SPD)."""
    rng = np.random.default_rng(seed)
    n = 6 * n_blocks
    A = np.zeros((n, n))
    for i, j in block_pairs:
        assert i != j
        B = rng.normal(0, 1, (6, 6))
        A[6 * i:6 * i + 6, 6 * j:6 * j + 6] = B
        A[6 * j:6 * j + 6, 6 * i:6 * i + 6] = B.T
    for i in range(n_blocks):
        D = rng.normal(0, 1, (6, 6))
        A[6 * i:6 * i + 6, 6 * i:6 * i + 6] = D + D.T
    A[np.arange(n), np.arange(n)] = np.abs(A).sum(axis=1) + rng.uniform(0.5, 1.5, n)
    if bad_block is not None:
        s = slice(6 * bad_block, 6 * bad_block + 6)
        A[s, s] = -A[s, s]
    return A, rng.normal(0, 1, n)


def ring(n, closed=True):
    return [(i, i + 1) for i in range(n - 1)] + ([(n - 1, 0)] if closed else [])


def tree40():
    return [(v, (v - 1) // 3) for v in range(1, 40)]


def banded_ring300():
    e = ring(300) + [(i, i - 2) for i in range(2, 300)] + [(i, i - 5) for i in range(5, 300, 3)]
    return e


def residual_bound_ok(A, b, x):
    """|| b - A x ||_2 <= n gamma_{3n+1} ||A||_2 ||x||_2 in np.longdouble (the condition-free bound of DESIGN.md section 6j); returns
    (holds, ||r|| / (||A|| ||x||), the bound's factor)."""
    n = len(b)
    u = 2.0 ** -53
    gamma = (3 * n + 1) * u / (1 - (3 * n + 1) * u)
    Al, xl, bl = A.astype(np.longdouble), x.astype(np.longdouble), b.astype(np.longdouble)
    r = float(np.sqrt(np.sum((bl - Al @ xl) ** 2)))
    scale = float(np.linalg.norm(A, 2)) * float(np.sqrt(np.sum(xl ** 2)))
    return r <= n * gamma * scale, r / scale, n * gamma
