"""Test support of the resident table's keyframe rows: builds tests/cpu_harness/mapdb_rows_check.cpp without sanitizers to obtain its
seeded operation sequence and counter trace (the GPU test replays both through the real handle), and builds and binds the CPU
restatement of the two local-map queries, tests/localmap_ref/localmap_ref.cpp.  Every comparison is exact."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from mapdb_support import check_ops
from mapmaint_support import ROOT, _flags

CHECK_SRC = os.path.join(ROOT, "tests", "cpu_harness", "mapdb_rows_check.cpp")
REF_SRC = os.path.join(ROOT, "tests", "localmap_ref", "localmap_ref.cpp")
TRACE_FIELDS = ("round", "n_keyframes", "n_entries", "pool_used", "pool_capacity", "repacks_kept", "repacks_grown", "header_growths",
                "header_capacity", "last_row_sync_bytes", "last_row_sync_records")
SEQUENCE_CAPACITIES = (640, 48, 4096)   # points, keyframes, observations: the row headers start at 48 slots, the row pool at 4096 entries
SEQUENCE_POINTS = 500                   # the check program's rows name point slots 0 .. 499
_REF = None
_VP, _I = C.c_void_p, C.c_int32


def parse_trace(lines):
    out = []
    for ln in lines:
        w = ln.split()
        assert w[0] == "trace" and len(w) == 1 + len(TRACE_FIELDS), ln
        out.append(dict(zip(TRACE_FIELDS, map(int, w[1:]))))
    return out


def sequence(tmp):
    """Runs the check program and returns its operations, one list per round: ("R", kf_slots, rows), ("E", kf, idx, slot), each round
    closed by ("S", trace)."""
    lines = check_ops(CHECK_SRC, tmp)
    rounds, cur, at = [], [], 0
    while at < len(lines):
        w = lines[at].split()
        at += 1
        if w[0] == "S":
            cur.append(("S", parse_trace([lines[at]])[0]))
            at += 1
            rounds.append(cur)
            cur = []
            continue
        n = int(w[1])
        rows = [[int(v) for v in ln.split()] for ln in lines[at:at + n]]
        at += n
        if w[0] == "R":
            assert all(len(r) == 2 + r[1] for r in rows)
            cur.append(("R", np.array([r[0] for r in rows], np.int32), [np.array(r[2:], np.int32) for r in rows]))
        else:
            a = np.array(rows, np.int32).reshape(-1, 3)
            cur.append(("E", a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()))
    assert not cur
    return rounds


class RowModel:
    """The naive model: one array per keyframe slot."""

    def __init__(self):
        self.rows = []

    def apply(self, op):
        if op[0] == "R":
            for k, r in zip(op[1], op[2]):
                while len(self.rows) <= k:
                    self.rows.append(np.zeros(0, np.int32))
                self.rows[k] = np.array(r, np.int32)
        else:
            for k, i, v in zip(*op[1:]):
                self.rows[k][i] = v

    def send(self, db, op):
        if op[0] == "R":
            db.set_keyframe_rows(op[1], op[2])
        else:
            db.set_row_entries(*op[1:])


def same_rows(got, want, n_keyframes=None):
    """Exported rows against the model's; keyframe slots past the model's have no row."""
    n = len(got) if n_keyframes is None else n_keyframes
    assert len(got) == n and len(want) <= n
    for k in range(n):
        w = want[k] if k < len(want) else np.zeros(0, np.int32)
        assert np.array_equal(got[k], np.asarray(w, np.int32)), k


def _p(a):
    return a.ctypes.data_as(_VP) if a is not None else None


def ref():
    global _REF
    if _REF is None:
        out = os.path.join(tempfile.mkdtemp(prefix="localmapref"), "liblocalmapref.so")
        subprocess.check_call(["g++", *_flags(), "-shared", "-o", out, REF_SRC])
        L = C.CDLL(out)
        L.localmapref_points_of_keyframes.restype = C.c_int
        L.localmapref_points_of_keyframes.argtypes = [_I, _VP, _VP, _VP, _VP, _I, _VP, _I, _VP, _VP]
        L.localmapref_observer_counter.restype = C.c_int
        L.localmapref_observer_counter.argtypes = [_VP, _VP, _VP, _VP, _I, _VP, _VP, _VP]
        _REF = L
    return _REF


def ref_points_of_keyframes(rows, bad, kf_slots, seen_points=None):
    """rows: one array per keyframe slot (an export); bad [n_points].  Returns (slots, seen)."""
    lens = [len(r) for r in rows]
    start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    slot = np.ascontiguousarray(np.concatenate(list(rows) + [np.zeros(0, np.int32)]), np.int32)
    bad = np.ascontiguousarray(bad, np.uint8)
    kf = np.ascontiguousarray(kf_slots, np.int32).reshape(-1)
    seen = np.zeros(0, np.int32) if seen_points is None else np.ascontiguousarray(seen_points, np.int32).reshape(-1)
    room = max(1, sum(lens[k] for k in kf))
    out, flag = np.zeros(room, np.int32), np.zeros(room, np.uint8)
    n = ref().localmapref_points_of_keyframes(len(bad), _p(bad), _p(start), _p(slot), _p(kf), len(kf), _p(seen), len(seen), _p(out), _p(flag))
    return out[:n], flag[:n]


def ref_observer_counter(table, point_slots):
    """table: an ObservationTable (an export).  Returns (kf, weight, point_bad) of one list."""
    pts = np.ascontiguousarray(point_slots, np.int32).reshape(-1)
    kf, w, pb = np.zeros(max(table.n_keyframes, 1), np.int32), np.zeros(max(table.n_keyframes, 1), np.int32), np.zeros(max(len(pts), 1), np.uint8)
    n = ref().localmapref_observer_counter(_p(table.obs_start), _p(table.obs_kf), _p(table.bad), _p(pts), len(pts), _p(kf), _p(w), _p(pb))
    return kf[:n], w[:n], pb[:len(pts)]


def check_points_of_keyframes(db, kf_slots, seen_points=None, exported=None):
    """db.points_of_keyframes against the restatement on the exported table.  Returns the result."""
    rows = db.export_rows() if exported is None else exported[0]
    bad = db.export()["table"].bad if exported is None else exported[1]
    got = db.points_of_keyframes(kf_slots, seen_points)
    want, wseen = ref_points_of_keyframes(rows, bad, kf_slots, seen_points)
    assert got["status"] == 0 and got["count"] == len(want), (got["count"], len(want))
    assert np.array_equal(got["slots"], want) and np.array_equal(got["seen"], wseen)
    return got
