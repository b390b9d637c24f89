"""Map maintenance on the GPU: the three kernels against the CPU restatement (tests/mapmaint_ref/mapmaint_ref.cpp), exactly: integers,
status bytes and float bit patterns.  The shapes sit on the kernels' edges: a partial and a full wave and workgroup of points, spans of
0, 1, 63, 64, 65 and 300 observers, keyframe counts on both sides of the histogram window and past two windows, capacities that fit
exactly and miss by one, one candidate and 65."""
import numpy as np
import pytest

import mapmaint_support as S
from mapmaint_support import f32

pytestmark = pytest.mark.gpu


def _M():
    from ydorbslam_amd import map_maintenance as M
    return M


# ------------------------------------------------------------------------------------------------------------ normal and depth
SPANS = (5, 0, 1, 63, 64, 65, 300, 2, 7, 12)


def normal_scene(n_points, n_levels, seed=4):
    """n_points over 320 keyframes; point i has SPANS[i % 10] observers (distinct, shuffled), its reference keyframe first, last or in the
    middle of its span by i % 3, every seventh point (from 3) bad, and point 2 sits exactly on its second observer's centre."""
    M = _M()
    rng = np.random.default_rng(seed)
    n_kf = 320
    obs = [rng.permutation(n_kf)[:SPANS[i % len(SPANS)]].astype(np.int32) for i in range(n_points)]
    lev = [rng.integers(0, n_levels, len(o)).astype(np.uint8) for o in obs]
    bad = np.array([1 if i % 7 == 3 else 0 for i in range(n_points)], np.uint8)
    T = M.ObservationTable(n_kf, obs, lev, [rng.integers(0, 2, len(o)) for o in obs], bad)
    centre = rng.uniform(-4.0, 4.0, (n_kf, 3)).astype(f32)
    pos = (rng.uniform(-6.0, 6.0, (n_points, 3)) + np.array([0.0, 0.0, 12.0])).astype(f32)
    if n_points > 2:
        pos[2] = centre[obs[2][0]]                 # SPANS[2] = 1: the only observer
    if n_points > 8:
        pos[8] = centre[obs[8][1]]                 # the second of seven
    at = [(0, len(o) - 1, len(o) // 2)[i % 3] if len(o) else 0 for i, o in enumerate(obs)]
    ref_kf = np.array([int(o[a]) if len(o) else 0 for o, a in zip(obs, at)], np.int32)
    ref_level = np.array([int(l[a]) if len(l) else 0 for l, a in zip(lev, at)], np.uint8)
    return T, pos, centre, ref_kf, ref_level, S.scale_factors(1.2, n_levels)


@pytest.mark.parametrize("n_levels", [1, 8])
@pytest.mark.parametrize("n_points", [1, 63, 64, 65, 1000])
def test_normal_and_depth_equal_the_restatement(n_points, n_levels):
    M = _M()
    args = normal_scene(n_points, n_levels)
    want = S.ref_update_normal_depth(*args)
    got = M.update_normal_depth(*args)
    S.same_normal_depth(got, want)
    again = M.update_normal_depth(*args)
    S.same_normal_depth(again, got)
    if n_points > 8:
        assert {0, 1, 2} == set(want["status"].tolist())
        assert np.isnan(want["normal"][2]).all() and np.isnan(want["normal"][8]).any()      # the points on a centre
        assert np.isfinite(want["normal"][want["status"] == 0][3:]).any()


# ------------------------------------------------------------------------------------------------------------ covisibility
def covis_scene(n_kf, Q, seed=6):
    """36 points whose observers are drawn from the slots 0, W-1, W, 2W-1, 2W, n-1 (those below n_kf) and twenty random ones; three bad
    points.  Q queries on those same slots first (so a query's own slot is among its points' observers); list 0 names one point twice,
    list 1 is empty."""
    M = _M()
    W = M.COVIS_WINDOW
    rng = np.random.default_rng(seed + n_kf + Q)
    special = sorted({s for s in (0, W - 1, W, 2 * W - 1, 2 * W, n_kf - 1) if 0 <= s < n_kf})
    pool = np.array(sorted(set(special) | set(rng.integers(0, n_kf, 20).tolist())), np.int32)
    obs = []
    for i in range(36):
        m = int(rng.integers(1, min(8, len(pool)) + 1))
        o = rng.permutation(pool)[:m]
        if i % 4 == 0:
            o = np.unique(np.concatenate([o, special]))[::-1]          # every fourth point is seen from all the special slots
        obs.append(o.astype(np.int32))
    bad = np.zeros(36, np.uint8)
    bad[[5, 17, 30]] = 1
    T = M.ObservationTable(n_kf, obs, [np.zeros(len(o), np.uint8) for o in obs], None, bad)
    query = np.array([(special + pool.tolist())[q % (len(special) + len(pool))] for q in range(Q)], np.int32)
    lists = [rng.integers(0, 36, int(rng.integers(1, 30))).astype(np.int32) for _ in range(Q)]
    lists[0] = np.concatenate([lists[0], [0, 4, 4, 5]]).astype(np.int32)
    if Q > 1:
        lists[1] = np.zeros(0, np.int32)
    return T, query, lists


@pytest.mark.parametrize("Q", [1, 3, 70])
@pytest.mark.parametrize("n_kf", ["1", "2", "W-1", "W", "W+1", "2W+5"])
def test_covisibility_equals_the_restatement(n_kf, Q):
    M = _M()
    W = M.COVIS_WINDOW
    n = {"1": 1, "2": 2, "W-1": W - 1, "W": W, "W+1": W + 1, "2W+5": 2 * W + 5}[n_kf]
    T, query, lists = covis_scene(n, Q)
    want = S.ref_covisibility(T, query, lists)
    got = M.covisibility(T, query, lists)                              # the tight bound the wrapper computes
    S.same_covisibility(got, want)
    assert all(w["status"] == 0 for w in want)
    if n > 2:
        assert max(w["count"] for w in want) >= 3 and (Q == 1 or want[1]["count"] == 0)
    exact = [w["count"] for w in want]                                 # fits exactly
    S.same_covisibility(M.covisibility(T, query, lists, exact), S.ref_covisibility(T, query, lists, exact))
    short = [max(c - 1, 0) if q % 2 == 0 else c for q, c in enumerate(exact)]   # every other query one short
    want_short = S.ref_covisibility(T, query, lists, short)
    got_short = M.covisibility(T, query, lists, short)
    S.same_covisibility(got_short, want_short)
    for q, g in enumerate(got_short):
        over = q % 2 == 0 and exact[q] > 0
        assert g["status"] == (1 if over else 0) and g["count"] == exact[q]
        assert not over or (g["raw_kf"] == -1).all() and (g["raw_weight"] == -1).all()      # nothing written
    S.same_covisibility(M.covisibility(T, query, lists), got)         # identical calls, identical bytes


def test_covisibility_of_a_random_map_with_long_lists():
    """Lists longer than a workgroup (about 180 entries per keyframe, two keyframes with every point) and every keyframe a query."""
    M = _M()
    m = S.random_map(21, 40, 600, 1, 12, bad_share=0.1)
    lists = list(m["kf_points"])
    lists[3] = np.arange(600, dtype=np.int32)
    lists[4] = np.concatenate([np.arange(600), np.arange(600)]).astype(np.int32)
    q = np.arange(40, dtype=np.int32)
    S.same_covisibility(M.covisibility(m["table"], q, lists), S.ref_covisibility(m["table"], q, lists))


# ------------------------------------------------------------------------------------------------------------ redundancy
def test_redundancy_boundaries():
    M = _M()
    table, cand, lists, own, want = S.boundary_table()
    r = M.keyframe_redundancy(table, cand, lists, own)
    assert list(r["n_counted"]) == want["n_counted"] and list(r["n_redundant"]) == want["n_redundant"] and list(r["cull"]) == want["cull"]
    S.same_redundancy(r, S.ref_keyframe_redundancy(table, cand, lists, own))


@pytest.mark.parametrize("seed", S.CULLING_SEEDS)
def test_redundancy_equals_the_restatement_with_and_without_removed(seed):
    M = _M()
    m = S.culling_map(seed)
    T = m["table"]
    cand, lists, own = S.candidates(m)
    want = S.ref_keyframe_redundancy(T, cand, lists, own)
    got = M.keyframe_redundancy(T, cand, lists, own)
    S.same_redundancy(got, want)
    assert want["cull"].any() and not want["cull"].all()
    removed = np.zeros(T.n_keyframes, np.uint8)
    removed[cand[want["cull"] != 0][:3]] = 1
    S.same_redundancy(M.keyframe_redundancy(T, cand, lists, own, removed), S.ref_keyframe_redundancy(T, cand, lists, own, removed))
    S.same_redundancy(M.keyframe_redundancy(T, cand, lists, own, np.zeros(T.n_keyframes, np.uint8)), want)   # an empty mask = NULL
    S.same_redundancy(M.keyframe_redundancy(T, cand, lists, own), got)                                       # identical calls
    seq = S.ref_sequential_culling(T, cand, lists, own)
    msk = S.masked_culling(M.keyframe_redundancy, T, cand, lists, own)
    for k in ("verdict", "erased", "n_counted", "n_redundant"):
        assert np.array_equal(seq[k], msk[k]), k


@pytest.mark.parametrize("K", [1, 65])
def test_redundancy_candidate_counts_and_an_empty_list(K):
    """One candidate, and 65 (lists of 30 to 60 entries: most waves straddle two candidates) of which the third has no entries and is
    not culled (0 > 0.0 is false)."""
    M = _M()
    m = S.random_map(13, 80, 600, 1, 12, level_spread=1, bad_share=0.05)
    cand = np.arange(1, K + 1, dtype=np.int32)
    lists, own = [m["kf_points"][k] for k in cand], [m["kf_levels"][k] for k in cand]
    if K > 2:
        lists[2], own[2] = np.zeros(0, np.int32), np.zeros(0, np.uint8)
    removed = np.zeros(80, np.uint8)
    removed[[70, 71, 72, 73]] = 1
    for rem in (None, removed):
        want = S.ref_keyframe_redundancy(m["table"], cand, lists, own, rem)
        S.same_redundancy(M.keyframe_redundancy(m["table"], cand, lists, own, rem), want)
        assert want["n_counted"].max() > 20
        if K > 2:
            assert (want["n_counted"][2], want["n_redundant"][2], want["cull"][2]) == (0, 0, 0)
    empty = M.keyframe_redundancy(m["table"], cand, [np.zeros(0, np.int32)] * K, [np.zeros(0, np.uint8)] * K)
    assert not empty["n_counted"].any() and not empty["cull"].any()
