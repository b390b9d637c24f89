"""The CPU restatement of KeyFrameDatabase (tests/kfdb_ref/kfdb_ref.cpp) checked without a GPU: its scores against an independent
numpy statement, its lists against hand-worked cases, and the shared scenarios of tests/kfdb_support.py shown not to be trivial.  Also
the parts of the new ABI that need no device: the symbols, the unsupported scorings and the adapter's syntax."""
import os
import subprocess

import numpy as np
import pytest

from kfdb_support import ROOT, SCENARIOS, SCORINGS, STALE, UNWRITTEN, RefDatabase, World, growth_scenario, numpy_score, replay_ref, scenario


def vec(words, values=None):
    w = np.array(sorted(words), np.int32)
    v = np.full(len(w), 1.0 / max(len(w), 1)) if values is None else np.array(values, np.float64)
    return w, v


@pytest.mark.parametrize("scoring", sorted(SCORINGS))
def test_scores_equal_numpy_statement(scoring):
    W = World(5, 60)
    db = RefDatabase(scoring)
    ids = [db.add(v) for v in W.vectors]
    shared = 0
    for _ in range(6):
        q = W.query(2)
        for k in ids:
            a, b = db.score(q, k), numpy_score(q, W.vectors[k], scoring)
            assert np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64), (scoring, k, a, b)
            shared += len(np.intersect1d(q[0], W.vectors[k][0])) > 1
    assert shared > 50   # sums of several terms, not single products


def test_score_corner_values():
    db = RefDatabase("L1_NORM")
    k = db.add(vec([1, 2]))
    s = db.score(vec([7, 8]), k)
    assert s == 0.0 and np.signbit(s)                 # -(+0.0) / 2.0: the sign of a zero sum is kept
    assert db.score(vec([1, 2]), k) == 1.0            # identical L1-normalised vectors
    d2 = RefDatabase("L2_NORM")
    k2 = d2.add(vec([1], [1.5]))
    assert d2.score(vec([1], [1.0]), k2) == 1.0       # DBoW's `>= 1` guard
    d3 = RefDatabase("CHI_SQUARE")
    k3 = d3.add(vec([1, 2], [0.5, -0.25]))
    assert d3.score(vec([1, 2], [0.5, 0.25]), k3) == 2.0 * (0.25 / 1.0)   # the word with vi + wi == 0 is left out


@pytest.mark.parametrize("mx,mn", [(1, 0), (3, 2), (5, 4), (6, 4), (10, 8), (11, 8), (20, 16), (21, 16)])
def test_min_common_words_is_a_truncated_float_product(mx, mn):
    """int minCommonWords = maxCommonWords * 0.8f: 5 * 0.8f rounds to 4.0f, 6 * 0.8f = 4.8000002f -> 4, 11 * 0.8f -> 8."""
    db = RefDatabase()
    top = db.add(vec(range(mx)))
    at_cut = db.add(vec(range(mn))) if mn else None          # words == minCommonWords: not scored (strict >)
    above = db.add(vec(range(mn + 1))) if mn + 1 < mx else None
    r = db.detect(vec(range(40)))
    assert r["stats"]["max_common"] == mx and r["stats"]["min_common"] == mn
    scored = 1 + (above is not None)
    assert r["stats"]["scored"] == scored and r["stats"]["sharing"] == scored + (at_cut is not None)
    assert top in r["candidates"]


def test_tie_on_max_scores_both():
    db = RefDatabase()
    a, b = db.add(vec([1, 2, 3])), db.add(vec([2, 3, 4]))
    r = db.detect(vec([1, 2, 3, 4]))
    assert r["stats"]["max_common"] == 3 and r["stats"]["scored"] == 2
    assert r["candidates"].tolist() == [a, b]          # both first share at word 1 resp. 2: order by first shared word


def test_list_order_is_first_shared_word_then_add_sequence():
    db = RefDatabase()
    p, q = db.add(vec([9])), db.add(vec([3]))          # q is added later but shares the smaller word
    assert db.detect(vec([3, 9]))["candidates"].tolist() == [q, p]
    db2 = RefDatabase()
    x, y = db2.add(vec([5])), db2.add(vec([5]))
    assert db2.detect(vec([5]))["candidates"].tolist() == [x, y]
    db2.erase(x)
    z = db2.add(vec([5]))                              # erase, then add: the new entry goes to the end of the word's list
    assert db2.detect(vec([5]))["candidates"].tolist() == [y, z]


def test_neighbour_choice_is_strict_and_first_occurrence_wins():
    db = RefDatabase()
    a, b, c = db.add(vec([1, 2])), db.add(vec([1, 2])), db.add(vec([1, 2], [0.4, 0.6]))
    q = vec([1, 2])
    # equal scores: a neighbour that merely ties does not replace the key frame itself
    # (scores 1, 1, 0.9.  a and b accumulate 2.0 each and keep themselves; c's 0.9 is below 0.75 * 2.0.  With >= the result were [b, a].)
    db.set_covisibility(a, [b])
    db.set_covisibility(b, [a])
    r = db.detect(q)
    assert r["candidates"].tolist() == [a, b] and r["stats"]["retained"] == 2
    # a strictly better neighbour replaces the key frame: entries a (1 + 0.9, best a), b (1.0 < 0.75 * 1.9, dropped), c (0.9 + 1, best a);
    # a's second appearance is dropped
    db.set_covisibility(a, [c])
    db.set_covisibility(b, [])
    db.set_covisibility(c, [a])
    r = db.detect(q)
    assert r["stats"]["retained"] == 2 and r["candidates"].tolist() == [a]
    assert r["status"] == 0


def test_stale_and_unwritten_neighbour_scores():
    db = RefDatabase()
    big = db.add(vec(range(10)))
    small = db.add(vec([0, 20, 21, 22]))               # shares one word with the first query: below the cut, never scored
    db.set_covisibility(big, [small])
    q1 = vec(range(10))
    r = db.detect(q1)
    assert r["status"] == UNWRITTEN and r["candidates"].tolist() == [big]
    r = db.detect(vec([0, 20, 21, 22]))                # scores `small` (4 common words) and `big`... big has 1: not scored
    assert r["stats"]["scored"] == 1
    r = db.detect(q1)                                  # small is unscored again: its score of the second query is read
    assert r["status"] == STALE and r["stats"]["stale_reads"] == 1


def test_loop_form_connected_set_and_min_score():
    db = RefDatabase()
    a, b, c = db.add(vec([1, 2, 3])), db.add(vec([1, 2, 3], [0.2, 0.3, 0.5])), db.add(vec([1, 2, 3], [0.5, 0.3, 0.2]))
    q = vec([1, 2, 3])
    assert db.detect(q, [], 0.0)["candidates"].tolist() == [a, b, c]
    r = db.detect(q, [a], 0.0)                         # a never enters the list
    assert r["candidates"].tolist() == [b, c] and r["stats"]["sharing"] == 2
    assert a in r["diag"]                              # ... although its words are counted
    assert db.detect(q, [], 2.0)["candidates"].tolist() == []        # minScore empties lScoreAndMatch
    assert db.detect(q, [a, b, c], 0.0)["stats"]["sharing"] == 0
    # mLoopScore is stored before the minScore filter: a's neighbour b is below minScore, still added to a's accumulated score
    db.set_covisibility(a, [b])
    sb = np.float32(db.score(q, b))
    r = db.detect(q, [], float(np.nextafter(sb, np.float32(2))))
    assert r["candidates"].tolist() == [a] and r["stats"]["scored"] == 3


def test_empty_database_and_disjoint_query():
    db = RefDatabase()
    assert db.detect(vec([1, 2]))["candidates"].tolist() == [] and db.detect(vec([1, 2]), [], 0.0)["stats"]["sharing"] == 0
    db.add(vec([5, 6]))
    assert db.detect(vec([1, 2]))["candidates"].tolist() == []
    assert db.detect(vec([]))["candidates"].tolist() == []
    db.clear()
    assert db.detect(vec([5, 6]))["candidates"].tolist() == []


def test_generator_makes_places():
    W = World(3, 200)
    n = np.array([len(w) for w, _ in W.vectors])
    assert n.min() >= 50 and n.max() <= 1600 and len(W.subsets) >= 5
    for w, v in W.vectors[:20]:
        assert np.all(np.diff(w) > 0) and abs(v.sum() - 1.0) < 1e-12 and w.max() < W.vocab
    inside = [sum(W.place_of[m] == W.place_of[k] for m in W.covisibility(k)) / max(1, len(W.covisibility(k))) for k in range(0, 200, 7)]
    assert np.mean(inside) > 0.7


def test_scenarios_are_not_trivial():
    """On the restatement alone: the scenarios the GPU tests replay take every branch worth taking."""
    queries = multi = stale = unwritten = dedup = cut = 0
    for name, (n, seed) in SCENARIOS.items():
        for rec in replay_ref(scenario(n, seed), "L1_NORM"):
            if rec[0] == "score":
                continue
            for r in rec[1]:
                s = r["stats"]
                queries += 1
                multi += len(r["candidates"]) >= 2
                stale += bool(r["status"] & STALE)
                unwritten += bool(r["status"] & UNWRITTEN)
                dedup += s["retained"] > s["candidates"]
                cut += s["sharing"] > s["scored"]
    print("queries %d, with >= 2 candidates %d, stale %d, unwritten %d, de-duplicated %d, cut by minCommonWords %d"
          % (queries, multi, stale, unwritten, dedup, cut))
    assert queries > 1000 and 2 * multi >= queries   # over the whole set, the queries on the empty and one-key-frame databases included
    assert stale >= 1 and unwritten >= 1 and dedup >= 1 and cut >= 1


def test_growth_scenario_reads_scores_written_before_the_growth():
    """On the restatement alone: after the second add of growth_scenario (the one that grows the slot table and compacts the pool), the
    queries return lists and read relocalisation scores that an earlier query wrote; the very first of them can only read scores
    written before the growth."""
    ops = growth_scenario()
    assert [op[0] for op in ops].count("add") == 2
    recs = replay_ref(ops, "L1_NORM")
    n_before = sum(op[0] in ("reloc", "loop", "score") for op in ops[:max(i for i, op in enumerate(ops) if op[0] == "add")])
    assert n_before >= 1 and recs[n_before][0] == "reloc"
    after = [r for rec in recs[n_before:] if rec[0] != "score" for r in rec[1]]
    stale = sum(bool(r["status"] & STALE) for r in after)
    multi = sum(len(r["candidates"]) >= 2 for r in after)
    written = sum(r["stats"]["scored"] for rec in recs[:n_before] if rec[0] == "reloc" for r in rec[1])
    print("queries after the growth %d, stale %d, with >= 2 candidates %d; scores written before it %d" % (len(after), stale, multi, written))
    assert written >= 1 and stale >= 1 and multi >= 1
    assert recs[n_before][1][0]["status"] & STALE


def test_abi_symbols_and_unsupported_scorings():
    import ctypes as C
    import ydorbslam_amd as y
    y.build_library()
    L = C.CDLL(y.library_path())
    names = [n for n in y._lib.SYMBOLS if n.startswith("ydorb_kfdb_")]
    assert len(names) == 10
    for n in names:
        assert hasattr(L, n), n
    src = open(os.path.join(ROOT, "include", "ydorb", "c_api.h")).read()
    for n in names:
        assert n + "(" in src
    for s in ("KL", "BHATTACHARYYA"):   # refused before a device is looked for
        with pytest.raises(y.YdorbError, match="unsupported scoring"):
            y.KeyFrameDatabase(s)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(y.YdorbError, match="no CPU fallback"):
            y.KeyFrameDatabase("L1_NORM")


def test_adapter_syntax():
    h = os.path.join(ROOT, "tests", "cpu_harness")
    subprocess.check_call(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-I" + os.path.join(h, "mock"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(h, "kfdb_syntax_check.cpp")])
