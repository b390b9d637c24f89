"""ydorb_kfdb_* on the GPU against the CPU restatement (tests/kfdb_ref/kfdb_ref.cpp): candidate slots and their order, counts, status
words, the diagnostic common-word counts, and the bit patterns of the diagnostic float scores and of ydorb_kfdb_score's doubles.

Exact equality is derived, not measured: the common-word count is an integer; the score is the reference's sum over the common words
in ascending id, one IEEE double operation per step (the library is compiled with -ffp-contract=off, no lane adds anything for a word
that is not common, sqrt is correctly rounded); the thresholds are single float products; the neighbour accumulation is a float sum in
list order; maxima are order-free; the result order is an integer key (first common word, add sequence)."""
import numpy as np
import pytest

from kfdb_support import SCENARIOS, SCORINGS, STALE, UNWRITTEN, World, compare, growth_scenario, replay_gpu, replay_ref, scenario

pytestmark = pytest.mark.gpu

SMALL = dict(slot_capacity=4, word_capacity=64)   # every scenario grows past its initial capacity


@pytest.mark.parametrize("scoring", sorted(SCORINGS))
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_scenario_equals_restatement(name, scoring):
    """N in {0, 1, 37, 90, 150, 600, 3000}, Q in {1, 7, 64}, interleaved add / erase / set_covisibility / queries, batched calls."""
    n, seed = SCENARIOS[name]
    ops = scenario(n, seed)
    compare(replay_ref(ops, scoring), replay_gpu(ops, scoring, batch=True, **SMALL))


@pytest.mark.parametrize("name,scoring", [("n37", "L1_NORM"), ("n37", "CHI_SQUARE"), ("n3000", "L1_NORM"), ("n1", "L2_NORM"), ("n0", "DOT_PRODUCT")])
def test_one_by_one_equals_batch(name, scoring):
    """The same scenario with every query in a call of its own: the relocalisation scores carried between queries and across calls give
    the same results as the batches (both equal the restatement, which runs one query at a time)."""
    n, seed = SCENARIOS[name]
    ops = scenario(n, seed)
    want = replay_ref(ops, scoring, diag="all" if n < 100 else "last")
    single = replay_gpu(ops, scoring, batch=False)
    compare(want, single)
    batch = replay_gpu(ops, scoring, batch=True, **SMALL)
    for a, b in zip(single, batch):
        if a[0] == "score":
            assert np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
        else:
            for ra, rb in zip(a[1], b[1]):
                assert np.array_equal(ra["candidates"], rb["candidates"]) and ra["status"] == rb["status"] and ra["count"] == rb["count"]


def test_growth_after_use_equals_restatement():
    """The slot table grows past its first 64 slots while relocalisation scores are resident, and the pool is compacted over erased rows
    while the device's slot table lags behind the host's (growth_scenario); queries batched and one by one."""
    ops = growth_scenario()
    want = replay_ref(ops, "L1_NORM", diag="all")
    for batch in (True, False):
        sizes = []
        got = replay_gpu(ops, "L1_NORM", batch=batch, sizes=sizes, slot_capacity=1, word_capacity=1)
        assert len(sizes) == 2 and sizes[0][1] <= 64 and sizes[1][1] > 64
        compare(want, got)


def test_stale_and_unwritten_status_bits_are_raised():
    seen = 0
    for rec in replay_gpu(scenario(*SCENARIOS["n37"]), "L1_NORM"):
        if rec[0] == "reloc":
            for r in rec[1]:
                seen |= r["status"]
    assert seen & STALE and seen & UNWRITTEN


def test_hand_cases_on_the_device():
    """The hand-worked cases of tests/test_kfdb_cpu.py through the product."""
    import ydorbslam_amd as y

    def vec(words, values=None):
        w = np.array(sorted(words), np.int32)
        return w, (np.full(len(w), 1.0 / max(len(w), 1)) if values is None else np.array(values, np.float64))

    db = y.KeyFrameDatabase("L1_NORM", slot_capacity=1, word_capacity=1)
    assert db.size() == (0, 0)
    r = db.detect_reloc([vec([1, 2])])
    assert r["counts"].tolist() == [0]
    p, q = db.add([vec([9]), vec([3])]).tolist()
    assert db.detect_reloc([vec([3, 9])])["candidates"][0].tolist() == [q, p]   # first shared word, then add sequence
    db.erase([p])
    z = int(db.add([vec([9])])[0])
    assert z == p and db.size() == (2, 2)                                       # the slot is reused ...
    r = db.detect_reloc([vec([9]), vec([3, 9]), vec([70])], diag=True)
    assert [c.tolist() for c in r["candidates"]] == [[z], [q, z], []]
    assert r["diag_words"].tolist() == [0, 0]
    s = db.score(vec([7, 8]), [q, z])
    assert np.all(s == 0.0) and np.all(np.signbit(s))                           # -(+0.0) / 2.0
    assert db.score(vec([3]), [q]).tolist() == [1.0]
    # cand_cap smaller than the result: the first entries, the full count
    r = db.detect_reloc([vec([3, 9])], cand_cap=1)
    assert r["counts"].tolist() == [2] and r["candidates"][0].tolist() == [q]
    # loop form: connected set, minScore
    assert db.detect_loop([vec([3, 9])], [[q]], 0.0)["candidates"][0].tolist() == [z]
    assert db.detect_loop([vec([3, 9])], [[]], 0.9)["candidates"][0].tolist() == []
    db.clear()
    assert db.size() == (0, 0) and db.detect_reloc([vec([3, 9])])["counts"].tolist() == [0]
    with pytest.raises(y.YdorbError, match="ascending"):
        db.add([(np.array([5, 5], np.int32), np.array([0.5, 0.5]))])
    with pytest.raises(y.YdorbError, match="not in the database"):
        db.erase([0])
    db.close()


@pytest.mark.parametrize("scoring", ["KL", "BHATTACHARYYA"])
def test_log_based_scorings_are_refused(scoring):
    import ydorbslam_amd as y
    with pytest.raises(y.YdorbError, match="unsupported scoring"):
        y.KeyFrameDatabase(scoring)


def test_long_rows_and_long_query():
    """Rows and a query near the 8192-word limit (many 64-word chunks per row), against the numpy statement."""
    import ydorbslam_amd as y
    from kfdb_support import numpy_score
    rng = np.random.default_rng(3)

    def big(n):
        w = np.sort(rng.choice(20000, n, replace=False)).astype(np.int32)
        v = rng.gamma(2.0, 1.0, n)
        return w, v / v.sum()

    rows = [big(n) for n in (8192, 5000, 64, 65, 1, 63)]
    qv = big(8192)
    for scoring in sorted(SCORINGS):
        db = y.KeyFrameDatabase(scoring)
        slots = db.add(rows)
        got = db.score(qv, slots)
        want = np.array([numpy_score(qv, r, scoring) for r in rows])
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), scoring
        db.close()
    with pytest.raises(y.YdorbError, match="at most 8192"):
        y.KeyFrameDatabase().detect_reloc([big(8193)])
