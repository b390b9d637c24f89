"""Test support of the resident table's point attributes: builds tests/cpu_harness/mapdb_attr_check.cpp without sanitizers to obtain
its seeded operation sequence and counter trace (the GPU test replays both through the real handle), keeps the naive model (one record
per slot, changed at once by every operation), and gathers the YdMapPointTable the flat entries would be given from a handle's
exports.  Every comparison is exact."""
import os

import numpy as np

from mapdb_support import check_ops
from mapmaint_support import ROOT

CHECK_SRC = os.path.join(ROOT, "tests", "cpu_harness", "mapdb_attr_check.cpp")
TRACE_FIELDS = ("round", "enabled", "growths", "capacity", "last_attr_sync_bytes", "last_attr_sync_records", "n_points")
SEQUENCE_CAPACITIES = (64, 4, 1024)   # the Db of the check program: points (kPointCap), keyframes, observations
GEOMETRY, DESCRIPTOR = 1, 2           # the flag byte
NO_ATTRIBUTES = 7                     # YDORB_FRUSTUM_NO_ATTRIBUTES
f32 = np.float32


def parse_trace(lines):
    out = []
    for ln in lines:
        w = ln.split()
        assert w[0] == "trace" and len(w) == 1 + len(TRACE_FIELDS), ln
        out.append(dict(zip(TRACE_FIELDS, map(int, w[1:]))))
    return out


def sequence(tmp):
    """Runs the check program and returns its operations, one list per round: ("P", slots, bad), ("A", slots, groups, geometry [n, 5]
    float32 or None, desc [n, 32] or None), each round closed by ("S", trace)."""
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
        rows = [ln.split() for ln in lines[at:at + n]]
        at += n
        slots = np.array([int(r[0]) for r in rows], np.int32)
        if w[0] == "P":
            cur.append(("P", slots, np.array([int(r[1]) for r in rows], np.uint8)))
        else:
            groups = int(w[2])
            geo = np.array([[int(x, 16) for x in r[1:6]] for r in rows], np.uint32).view(f32).reshape(n, 5) if groups & GEOMETRY else None
            desc = np.stack([np.frombuffer(bytes.fromhex(r[-1]), np.uint8) for r in rows]) if groups & DESCRIPTOR else None
            cur.append(("A", slots, groups, geo, desc))
    assert not cur
    return rounds


class AttrModel:
    """The naive model: per slot normal, distances, descriptor and flags; a slot never set or erased is all zero."""

    def __init__(self):
        self.normal, self.mn, self.mx = np.zeros((0, 3), f32), np.zeros(0, f32), np.zeros(0, f32)
        self.desc, self.flags = np.zeros((0, 32), np.uint8), np.zeros(0, np.uint8)

    def grow(self, n):
        k = n - len(self.flags)
        if k > 0:
            self.normal, self.mn, self.mx = np.concatenate([self.normal, np.zeros((k, 3), f32)]), np.concatenate([self.mn, np.zeros(k, f32)]), np.concatenate([self.mx, np.zeros(k, f32)])
            self.desc, self.flags = np.concatenate([self.desc, np.zeros((k, 32), np.uint8)]), np.concatenate([self.flags, np.zeros(k, np.uint8)])

    def set_points(self, slots, bad):
        self.grow(int(np.max(slots)) + 1)
        for s in np.asarray(slots)[np.asarray(bad) != 0]:
            self.normal[s], self.mn[s], self.mx[s], self.desc[s], self.flags[s] = 0, 0, 0, 0, 0

    def set(self, slots, normal=None, mn=None, mx=None, desc=None):
        for i, s in enumerate(slots):          # one after the other: the last value of a repeated slot wins
            if normal is not None:
                self.normal[s], self.mn[s], self.mx[s] = normal[i], mn[i], mx[i]
                self.flags[s] |= GEOMETRY
            if desc is not None:
                self.desc[s] = desc[i]
                self.flags[s] |= DESCRIPTOR

    def check_export(self, db):
        got = db.export_attributes()
        assert np.array_equal(got["flags"], self.flags)
        for k, want in (("normal", self.normal), ("min_distance", self.mn), ("max_distance", self.mx)):
            assert np.array_equal(got[k].view(np.uint32), want.view(np.uint32)), k
        assert np.array_equal(got["desc"], self.desc)
        return got


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def gathered_table(db, slots):
    """(PointTable, has_observations, resident bad) of the listed slots, gathered in numpy from the handle's exports: row i = the
    resident values of slots[i], with 0.8f * minDistance and 1.2f * maxDistance as single float32 products."""
    from ydorbslam_amd.frustum import PointTable
    slots = np.asarray(slots, np.int64).reshape(-1)
    a, e = db.export_attributes(), db.export()
    spans = np.diff(np.asarray(e["table"].obs_start, np.int64))
    mn, mx = a["min_distance"][slots], a["max_distance"][slots]
    table = PointTable(e["pos"][slots], a["normal"][slots], f32(0.8) * mn, f32(1.2) * mx, mx, a["desc"][slots])
    return table, (spans[slots] > 0).astype(np.uint8), np.asarray(e["table"].bad, np.uint8)[slots], a["flags"][slots]
