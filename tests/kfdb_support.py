"""Test support of the key-frame database: builds the CPU restatement tests/kfdb_ref/kfdb_ref.cpp with oracle/Makefile's compiler flags,
states the four scores independently in numpy, generates "places" (groups of key frames drawing words from overlapping subsets of a
large vocabulary) and the shared scenarios, and replays a scenario on the restatement or on the product.

A scenario is a list of operations on key frames known by their creation index (= the restatement's id):
  ("add", [(words, values), ...])            ("erase", [kf, ...])           ("clear",)
  ("covis", [kf, ...], [[kf, ...], ...])     ("score", (words, values), [kf, ...])
  ("reloc", [query, ...])                    ("loop", [query, ...], [[connected kf, ...], ...], [minScore, ...])"""
import ctypes as C
import os
import re
import shlex
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "kfdb_ref", "kfdb_ref.cpp")
_REF = None

SCORINGS = {"L1_NORM": 0, "L2_NORM": 1, "CHI_SQUARE": 2, "DOT_PRODUCT": 5}
STALE, UNWRITTEN = 1, 2


def _flags():
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return shlex.split(re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1))


def ref():
    global _REF
    if _REF is None:
        out = os.path.join(tempfile.mkdtemp(prefix="kfdbref"), "libkfdbref.so")
        subprocess.check_call(["g++", *_flags(), "-shared", "-o", out, SRC, "-lm"])
        L = C.CDLL(out)
        VP = C.c_void_p
        L.kfdbref_create.restype = VP
        L.kfdbref_create.argtypes = [C.c_int]
        L.kfdbref_destroy.restype = None
        L.kfdbref_destroy.argtypes = [VP]
        L.kfdbref_add.restype = C.c_long
        L.kfdbref_add.argtypes = [VP, VP, VP, C.c_int]
        L.kfdbref_erase.argtypes = [VP, C.c_long]
        L.kfdbref_clear.restype = None
        L.kfdbref_clear.argtypes = [VP]
        L.kfdbref_set_covisibility.argtypes = [VP, C.c_long, VP, C.c_int]
        L.kfdbref_score.restype = C.c_double
        L.kfdbref_score.argtypes = [VP, VP, VP, C.c_int, C.c_long]
        L.kfdbref_detect.argtypes = [VP, C.c_int, VP, VP, C.c_int, VP, C.c_int, C.c_float] + [VP] * 6
        _REF = L
    return _REF


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _wv(vec):
    return np.ascontiguousarray(vec[0], np.int32), np.ascontiguousarray(vec[1], np.float64)


class RefDatabase:
    """The restatement behind Python calls.  Key frames are known by the id add() returns (0, 1, 2, ... in creation order)."""

    def __init__(self, scoring="L1_NORM"):
        self._h = C.c_void_p(ref().kfdbref_create(SCORINGS[scoring]))
        self.ids = set()

    def __del__(self):
        if getattr(self, "_h", None):
            ref().kfdbref_destroy(self._h)
            self._h = None

    def add(self, vec):
        w, v = _wv(vec)
        i = int(ref().kfdbref_add(self._h, _p(w), _p(v), len(w)))
        self.ids.add(i)
        return i

    def erase(self, i):
        assert ref().kfdbref_erase(self._h, i) == 0
        self.ids.discard(i)

    def clear(self):
        ref().kfdbref_clear(self._h)
        self.ids.clear()

    def set_covisibility(self, i, neigh):
        nb = np.ascontiguousarray(neigh, np.int64)
        assert ref().kfdbref_set_covisibility(self._h, i, _p(nb), len(nb)) == 0

    def score(self, vec, i):
        w, v = _wv(vec)
        return float(ref().kfdbref_score(self._h, _p(w), _p(v), len(w), i))

    def detect(self, vec, connected=None, min_score=0.0, diag=True):
        """One query.  connected None: detectRelocalizationCandidates; else detectLoopCandidates.  Returns dict(candidates (ids), stats,
        status [, diag {id: (common words, float score)}: costly, it scores every key frame that shares a word])."""
        w, v = _wv(vec)
        n = max(len(self.ids), 1)
        out = np.zeros(n, np.int64)
        stats = np.zeros(8, np.int32)
        did, dw, ds, nd = np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(1, np.int32)
        conn = np.ascontiguousarray(connected if connected is not None else [], np.int64)
        cnt = ref().kfdbref_detect(self._h, int(connected is not None), _p(w), _p(v), len(w), _p(conn), len(conn), float(min_score), _p(out),
                                   _p(stats), _p(did) if diag else None, _p(dw), _p(ds), _p(nd))
        k = int(nd[0])
        names = ("sharing", "scored", "retained", "candidates", "max_common", "min_common", "status", "stale_reads")
        r = dict(candidates=out[:cnt].copy(), stats=dict(zip(names, (int(s) for s in stats))), status=int(stats[6]))
        if diag:
            r["diag"] = {int(i): (int(a), np.float32(b)) for i, a, b in zip(did[:k], dw[:k], ds[:k])}
        return r


# ------------------------------------------------------------------------------------------------ the scores, stated independently
def numpy_score(a, b, scoring):
    """DBoW's score of two sparse vectors: the common words by set intersection, the sum in ascending word order in Python floats
    (IEEE doubles, one operation at a time)."""
    wa, va = _wv(a)
    wb, vb = _wv(b)
    _, ia, ib = np.intersect1d(wa, wb, assume_unique=True, return_indices=True)   # ascending
    s = 0.0
    for x, y in zip(va[ia].tolist(), vb[ib].tolist()):
        if scoring == "L1_NORM":
            s += abs(x - y) - abs(x) - abs(y)
        elif scoring == "CHI_SQUARE":
            if x + y != 0.0:
                s += x * y / (x + y)
        else:
            s += x * y
    if scoring == "L1_NORM":
        return -s / 2.0
    if scoring == "L2_NORM":
        return 1.0 if s >= 1 else 1.0 - float(np.sqrt(np.float64(1.0 - s)))
    if scoring == "CHI_SQUARE":
        return 2.0 * s
    return s


# -------------------------------------------------------------------------------------------------------------------- the generator
def _vector(rng, subset, n, vocab, stray=0.05):
    n = int(min(n, len(subset)))
    w = rng.choice(subset, n, replace=False)
    k = int(stray * n)
    if k:
        w = np.concatenate([w, rng.integers(0, vocab, k)])
    w = np.unique(w).astype(np.int32)
    v = rng.gamma(2.0, 1.0, len(w)) + 1e-3
    return w, v / v.sum()   # L1-normalised


class World:
    """Places: each has a word subset that overlaps its predecessor's by a quarter; its key frames draw 50-1500 words from it."""

    def __init__(self, seed, n_kf, vocab=300000, place_size=(12, 40), words=(50, 1500)):
        rng = self.rng = np.random.default_rng(seed)
        self.vocab = vocab
        self.subsets, self.place_of, self.vectors, self.members = [], [], [], []
        prev = None
        while len(self.vectors) < n_kf:
            size = int(rng.integers(place_size[0], place_size[1] + 1))
            rich = int(rng.integers(words[0], words[1] + 1))
            sub = rng.integers(0, vocab, int(rich * 1.5) + 30)
            if prev is not None:
                sub = np.concatenate([sub, rng.choice(prev, len(prev) // 4, replace=False)])
            sub = np.unique(sub)
            p = len(self.subsets)
            self.subsets.append(sub)
            self.members.append([])
            for _ in range(min(size, n_kf - len(self.vectors))):
                n = int(np.clip(rich * rng.uniform(0.6, 1.0), words[0], words[1]))
                self.members[p].append(len(self.vectors))
                self.place_of.append(p)
                self.vectors.append(_vector(rng, sub, n, vocab))
            prev = sub

    def covisibility(self, k, outside=0.1):
        """Up to 10 neighbours of key frame k (index into self.vectors), mostly of its place."""
        rng = self.rng
        mates = [m for m in self.members[self.place_of[k]] if m != k]
        out = list(rng.permutation(mates)[:10]) if mates else []
        for i in range(len(out)):
            if rng.uniform() < outside:
                out[i] = int(rng.integers(0, len(self.vectors)))
        return [int(x) for x in out if x != k]

    def query(self, mix=2):
        """A frame that sees `mix` places at once (none when the world is empty: random words)."""
        rng = self.rng
        if not self.subsets:
            return _vector(rng, np.arange(1000), 200, self.vocab)
        ps = rng.integers(0, len(self.subsets), mix)
        sub = np.unique(np.concatenate([self.subsets[p] for p in ps]))
        n = int(np.clip(len(sub) * rng.uniform(0.3, 0.6), 50, 1500))
        return _vector(rng, sub, n, self.vocab)


def scenario(n_kf, seed, q_sizes=(1, 7, 64)):
    """add (in three batches) / covisibility / queries of every batch size in both forms / score / erase + add (slot reuse, changed list
    order) / covisibility / queries again.  Key-frame numbers are creation indices."""
    W = World(seed, n_kf + max(2, n_kf // 10))
    rng = W.rng
    ops = []
    first = list(range(n_kf))
    for part in np.array_split(np.arange(n_kf), 3):
        if len(part):
            ops.append(("add", [W.vectors[k] for k in part]))
    live = list(first)
    if live:
        ops.append(("covis", live[:], [W.covisibility(k) for k in live]))

    def queries(form, Q):
        qs = [W.query(int(rng.integers(1, 4))) for _ in range(Q)]
        if form == "reloc":
            return ("reloc", qs)
        conn, ms = [], []
        for _ in range(Q):
            c = [int(x) for x in rng.choice(live, min(len(live), int(rng.integers(0, 15))), replace=False)] if live else []
            conn.append(c)
            ms.append(float(np.float32(rng.choice([0.0, 0.005, 0.02, 0.9]))))
        return ("loop", qs, conn, ms)

    for Q in q_sizes:
        ops.append(queries("reloc", Q))
        ops.append(queries("loop", Q))
    if live:
        ops.append(("score", W.query(1), [int(x) for x in rng.choice(live, min(len(live), 20), replace=False)]))
        # erase a tenth, add as many new ones: the new key frames take the freed slots and sit at the END of every inverted-file list
        gone = sorted(int(x) for x in rng.choice(live, max(1, n_kf // 10), replace=False))
        ops.append(("erase", gone))
        live = [k for k in live if k not in set(gone)]
        new = list(range(n_kf, n_kf + len(gone)))
        ops.append(("add", [W.vectors[k] for k in new]))
        live += new
        # the restatement's ids follow creation order, and so do the world's indices: neighbours are named by them; erased ones drop out
        touched = new + [int(x) for x in rng.choice(live, min(len(live), 8), replace=False)]
        ops.append(("covis", touched, [[m for m in W.covisibility(k) if m in set(live)] for k in touched]))
        for Q in (q_sizes[0], q_sizes[-1]):
            ops.append(queries("reloc", Q))
            ops.append(queries("loop", Q))
        ops.append(("score", W.query(2), live[-10:]))
    return ops


def growth_scenario(seed=22, n_first=40, n_second=50):
    """Growth after use, for a database created with slot_capacity=1, word_capacity=1 (64 slots, 1024 words): add n_first key frames in one
    call / covisibility / relocalisation queries (they write scores) / erase every third key frame / add n_second key frames in one call /
    covisibility / queries in both forms / score.  The second add takes the freed slots and n_second - n_first // 3 more, which passes 64
    slots while scores are resident; it holds more words than the first, and the pool's capacity is twice what the first stored, so the
    pool is compacted over erased rows while the device's slot table lags behind the host's.  Both batches draw from every place of
    the world (a random order of creation), so the new key frames have old ones as neighbours and the later queries read old scores."""
    n = n_first + n_second
    W = World(seed, n)
    rng = W.rng
    world_of = [int(x) for x in rng.permutation(n)]            # creation index -> index into W.vectors
    kf_of = {w: k for k, w in enumerate(world_of)}

    def words(kfs):
        return sum(len(W.vectors[world_of[k]][0]) for k in kfs)

    def covis(kfs, live):
        return ("covis", list(kfs), [[kf_of[m] for m in W.covisibility(world_of[k]) if kf_of[m] in live] for k in kfs])

    def reloc(Q):
        return ("reloc", [W.query(int(rng.integers(1, 4))) for _ in range(Q)])

    first, second = list(range(n_first)), list(range(n_first, n))
    gone = first[::3]
    live = set(first) - set(gone)
    assert len(second) > len(live) and n_first + len(second) - len(gone) > 64
    assert words(first) > 1024 and words(second) > words(first)
    ops = [("add", [W.vectors[world_of[k]] for k in first]), covis(first, set(first)), reloc(6), ("erase", gone),
           ("add", [W.vectors[world_of[k]] for k in second])]
    live |= set(second)
    ops.append(covis(sorted(live), live))
    ops.append(reloc(7))
    Q = 5
    conn = [[int(x) for x in rng.choice(sorted(live), int(rng.integers(0, 15)), replace=False)] for _ in range(Q)]
    ops.append(("loop", [W.query(2) for _ in range(Q)], conn, [float(np.float32(rng.choice([0.0, 0.005, 0.02]))) for _ in range(Q)]))
    ops.append(reloc(1))
    ops.append(("score", W.query(2), sorted(live)[::4]))
    return ops


# name -> (key frames, seed).  tests/test_kfdb_cpu.py asserts on the restatement that these are not trivial.  n0 and n1 cannot return two
# candidates; n90, n150 and n600 are there so that, over the whole set, at least half of the queries still do.
SCENARIOS = {"n0": (0, 11), "n1": (1, 12), "n37": (37, 13), "n90": (90, 17), "n150": (150, 15), "n600": (600, 16), "n3000": (3000, 14)}


def replay_ref(ops, scoring, diag="last"):
    """The scenario on the restatement: one record per query / score operation.  diag: "last" keeps the diagnostics of the last query
    of every operation (what a batched call returns), "all" those of every query."""
    db = RefDatabase(scoring)
    out = []
    for op in ops:
        if op[0] == "add":
            for v in op[1]:
                db.add(v)
        elif op[0] == "erase":
            for k in op[1]:
                db.erase(k)
        elif op[0] == "clear":
            db.clear()
        elif op[0] == "covis":
            for k, nb in zip(op[1], op[2]):
                db.set_covisibility(k, nb)
        elif op[0] == "score":
            out.append(("score", np.array([db.score(op[1], k) for k in op[2]], np.float64)))
        elif op[0] == "reloc":
            out.append(("reloc", [db.detect(q, diag=diag == "all" or i == len(op[1]) - 1) for i, q in enumerate(op[1])]))
        elif op[0] == "loop":
            out.append(("loop", [db.detect(q, c, m, diag == "all" or i == len(op[1]) - 1) for i, (q, c, m) in enumerate(zip(op[1], op[2], op[3]))]))
    return out


def replay_gpu(ops, scoring, batch=True, sizes=None, **create):
    """The scenario on the product; key frames are mapped to slots here.  batch=False issues every query in a call of its own.
    Records as replay_ref's, with key-frame numbers in place of slots; the diagnostics are those of the last query of each operation.
    sizes: a list that receives db.size() after every add."""
    from ydorbslam_amd.kfdb import KeyFrameDatabase
    db = KeyFrameDatabase(scoring, **create)
    slot_of, kf_of, created = {}, {}, 0
    out = []

    def result(r, i, with_diag):
        d = dict(candidates=np.array([kf_of[int(s)] for s in r["candidates"][i]], np.int64), count=int(r["counts"][i]), status=int(r["status"][i]))
        if with_diag:
            d["diag"] = {kf_of[s]: (int(r["diag_words"][s]), np.float32(r["diag_score"][s])) for s in np.nonzero(r["diag_words"])[0].tolist()}
        return d

    for op in ops:
        if op[0] == "add":
            for s in db.add(op[1]).tolist():
                slot_of[created] = s
                kf_of[s] = created
                created += 1
            if sizes is not None:
                sizes.append(db.size())
        elif op[0] == "erase":
            db.erase([slot_of[k] for k in op[1]])
            for k in op[1]:
                del kf_of[slot_of.pop(k)]
        elif op[0] == "clear":
            db.clear()
            slot_of.clear()
            kf_of.clear()
        elif op[0] == "covis":
            db.set_covisibility([slot_of[k] for k in op[1]], [[slot_of[m] for m in nb if m in slot_of] for nb in op[2]])
        elif op[0] == "score":
            out.append(("score", db.score(op[1], [slot_of[k] for k in op[2]])))
        else:
            Q = len(op[1])
            groups = [list(range(Q))] if batch else [[i] for i in range(Q)]
            recs = []
            for g in groups:
                qs = [op[1][i] for i in g]
                if op[0] == "reloc":
                    r = db.detect_reloc(qs, diag=True)
                else:
                    r = db.detect_loop(qs, [[slot_of[k] for k in op[2][i] if k in slot_of] for i in g], [op[3][i] for i in g], diag=True)
                recs += [result(r, j, j == len(g) - 1) for j in range(len(g))]
            out.append((op[0], recs))
    db.close()
    return out


def compare(ref_out, gpu_out):
    """Every record of a replay: candidates and their order, counts, status words, diagnostics (bit patterns), score doubles (bit
    patterns).  Raises AssertionError naming the operation and query."""
    assert len(ref_out) == len(gpu_out)
    for n, (a, b) in enumerate(zip(ref_out, gpu_out)):
        assert a[0] == b[0]
        if a[0] == "score":
            assert np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64)), "op %d (score): %r vs %r" % (n, a[1], b[1])
            continue
        assert len(a[1]) == len(b[1])
        for q, (ra, rb) in enumerate(zip(a[1], b[1])):
            where = "op %d (%s) query %d" % (n, a[0], q)
            if "diag" in rb and "diag" in ra:   # first, to localise a mismatch
                assert set(ra["diag"]) == set(rb["diag"]), where + ": key frames sharing a word differ"
                for k, (w, s) in ra["diag"].items():
                    assert rb["diag"][k][0] == w, where + ": common words of key frame %d: %d vs %d" % (k, w, rb["diag"][k][0])
                    assert np.float32(s).view(np.uint32) == np.float32(rb["diag"][k][1]).view(np.uint32), \
                        where + ": score of key frame %d: %r vs %r" % (k, s, rb["diag"][k][1])
            assert rb["count"] == len(ra["candidates"]), where + ": %d candidates vs %d" % (len(ra["candidates"]), rb["count"])
            assert np.array_equal(ra["candidates"], rb["candidates"]), where + ": %r vs %r" % (ra["candidates"], rb["candidates"])
            assert ra["status"] == rb["status"], where + ": status %d vs %d" % (ra["status"], rb["status"])
