"""ctypes mirror of the key-frame database part of the C ABI (include/ydorb/c_api.h, "KeyFrameDatabase"): KeyFrameDatabase::add / erase /
clear / detectRelocalizationCandidates / detectLoopCandidates and DBoW3::Vocabulary::score on the GPU.  Restates ORB-SLAM2's
KeyFrameDatabase.cc, which YDORBSLAM renames to keyFrameDatabase.*; DESIGN.md section 6e lists the assumed spellings.  A key frame is
known by its slot; a BowVector is a pair (word ids int32 ascending, values float64), as Vocabulary.transform returns it."""
import ctypes as C

import numpy as np

from ._lib import check, lib

SCORING = {"L1_NORM": 0, "L2_NORM": 1, "CHI_SQUARE": 2, "KL": 3, "BHATTACHARYYA": 4, "DOT_PRODUCT": 5}
STALE_SCORE, UNWRITTEN_SCORE = 1, 2
N_NEIGH = 10


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _csr(vectors):
    """[(words, values), ...] -> start [n + 1], words, values (contiguous)."""
    start = np.zeros(len(vectors) + 1, np.int32)
    for i, (w, _) in enumerate(vectors):
        start[i + 1] = start[i] + len(w)
    word = np.zeros(max(int(start[-1]), 1), np.int32)
    val = np.zeros(max(int(start[-1]), 1), np.float64)
    for i, (w, v) in enumerate(vectors):
        word[start[i]:start[i + 1]] = w
        val[start[i]:start[i + 1]] = v
    return start, word, val


class KeyFrameDatabase:
    """A key-frame database resident on the GPU."""

    def __init__(self, scoring="L1_NORM", device=0, slot_capacity=1024, word_capacity=1 << 20):
        self._L = lib()
        self._h = C.c_void_p()
        self.scoring = SCORING[scoring] if isinstance(scoring, str) else int(scoring)
        check(self._L.ydorb_kfdb_create(int(device), self.scoring, int(slot_capacity), int(word_capacity), C.byref(self._h)))

    def close(self):
        if self._h:
            self._L.ydorb_kfdb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def add(self, vectors):
        """add() for each (words, values) in order; returns their slots."""
        if not len(vectors):
            return np.zeros(0, np.int32)
        start, word, val = _csr(vectors)
        slots = np.zeros(len(vectors), np.int32)
        check(self._L.ydorb_kfdb_add(self._h, _p(start), _p(word), _p(val), len(vectors), _p(slots)))
        return slots

    def erase(self, slots):
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        check(self._L.ydorb_kfdb_erase(self._h, _p(slots), len(slots)))

    def clear(self):
        check(self._L.ydorb_kfdb_clear(self._h))

    def size(self):
        """(key frames in the database, slots in use)."""
        a, b = C.c_int32(), C.c_int32()
        check(self._L.ydorb_kfdb_size(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_covisibility(self, slots, neigh):
        """neigh [n][<=10]: getBestCovisibilityKeyFrames(10) of each slot, as slots."""
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        nb = np.full((len(slots), N_NEIGH), -1, np.int32)
        for i, row in enumerate(neigh):
            row = np.asarray(row, np.int32)[:N_NEIGH]
            nb[i, :len(row)] = row
        check(self._L.ydorb_kfdb_set_covisibility(self._h, _p(slots), _p(nb), len(slots)))

    def score(self, query, slots):
        """Vocabulary::score(query, key frame) per slot (float64)."""
        w = np.ascontiguousarray(query[0], np.int32)
        v = np.ascontiguousarray(query[1], np.float64)
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        out = np.zeros(len(slots), np.float64)
        check(self._L.ydorb_kfdb_score(self._h, _p(w), _p(v), len(w), _p(slots), len(slots), _p(out)))
        return out

    def _detect(self, queries, connected, min_score, cand_cap, diag):
        Q = len(queries)
        start, word, val = _csr(queries)
        n_slots = self.size()[1]
        cap = max(1, n_slots if cand_cap is None else int(cand_cap))
        cand = np.full((max(Q, 1), cap), -1, np.int32)
        counts = np.zeros(max(Q, 1), np.int32)
        status = np.zeros(max(Q, 1), np.int32)
        dw = np.zeros(max(n_slots, 1), np.int32) if diag else None
        ds = np.zeros(max(n_slots, 1), np.float32) if diag else None
        if connected is None:
            check(self._L.ydorb_kfdb_detect_reloc(self._h, _p(start), _p(word), _p(val), Q, _p(cand), cap, _p(counts), _p(status), _p(dw), _p(ds)))
        else:
            cs = np.zeros(Q + 1, np.int32)
            for i, c in enumerate(connected):
                cs[i + 1] = cs[i] + len(c)
            ck = np.zeros(max(int(cs[-1]), 1), np.int32)
            for i, c in enumerate(connected):
                ck[cs[i]:cs[i + 1]] = np.asarray(c, np.int32)
            ms = np.ascontiguousarray(np.broadcast_to(np.asarray(min_score, np.float32), (Q,)))
            check(self._L.ydorb_kfdb_detect_loop(self._h, _p(start), _p(word), _p(val), Q, _p(cs), _p(ck), _p(ms), _p(cand), cap, _p(counts),
                                                 _p(status), _p(dw), _p(ds)))
        out = [cand[q, :min(int(counts[q]), cap)].copy() for q in range(Q)]
        res = dict(candidates=out, counts=counts[:Q].copy(), status=status[:Q].copy())
        if diag:
            res["diag_words"], res["diag_score"] = dw[:n_slots], ds[:n_slots]
        return res

    def detect_reloc(self, queries, cand_cap=None, diag=False):
        """detectRelocalizationCandidates for each query (words, values) in order, in one call.  Returns dict(candidates = list of slot
        arrays in the reference's order, counts, status [, diag_words, diag_score of the last query])."""
        return self._detect(queries, None, None, cand_cap, diag)

    def detect_loop(self, queries, connected, min_score, cand_cap=None, diag=False):
        """detectLoopCandidates(pKF, minScore) per query; connected: per query the slots of pKF's connected key frames; min_score: float or
        one per query."""
        return self._detect(queries, list(connected), min_score, cand_cap, diag)
