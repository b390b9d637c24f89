"""Test support of the resident table's descriptor blocks and point views: builds tests/cpu_harness/mapdb_desc_check.cpp without
sanitizers to obtain its seeded operation sequence and counter trace (the GPU test replays both through the real handle), keeps the
naive model, and states the query's reference: oracle.orb_oracle.distinctive_descriptor on rows gathered in Python from the model's own
arrays.  Every comparison is exact."""
import os

import numpy as np

from mapdb_support import check_ops
from mapmaint_support import ROOT

CHECK_SRC = os.path.join(ROOT, "tests", "cpu_harness", "mapdb_desc_check.cpp")
TRACE_FIELDS = ("round", "n_views", "n_descriptors", "view_pool_used", "view_pool_capacity", "desc_pool_used", "desc_pool_capacity",
                "view_repacks_kept", "view_repacks_grown", "desc_repacks_kept", "desc_repacks_grown", "last_desc_sync_bytes", "last_desc_sync_records")
SEQUENCE_POINTS, SEQUENCE_KEYFRAMES = 200, 64     # the check program's kPoints / kKeyframes
SEQUENCE_RESERVE = (256, 512)                     # ... and its reserve(): views, descriptors
STAGE_ROWS = 128                                  # kStageRows of ydorbslam_amd/csrc/mapdb_desc_kernels.hip.h
UPDATED, BAD, NO_DESCRIPTORS, VIEW_OUT_OF_RANGE = 0, 1, 2, 3


def parse_trace(lines):
    out = []
    for ln in lines:
        w = ln.split()
        assert w[0] == "trace" and len(w) == 1 + len(TRACE_FIELDS), ln
        out.append(dict(zip(TRACE_FIELDS, map(int, w[1:]))))
    return out


def sequence(tmp):
    """Runs the check program and returns its operations, one list per round: ("P", n_points), ("B", kf_slots, blocks), ("V", slots,
    views), each round closed by ("S", trace)."""
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
        elif w[0] == "P":
            cur.append(("P", int(w[1])))
        else:
            n = int(w[1])
            rows = [ln.split() for ln in lines[at:at + n]]
            at += n
            if w[0] == "B":
                blocks = [np.frombuffer(bytes.fromhex(r[2]) if len(r) > 2 else b"", np.uint8).reshape(-1, 32) for r in rows]
                assert all(len(b) == int(r[1]) for b, r in zip(blocks, rows))
                cur.append(("B", np.array([int(r[0]) for r in rows], np.int32), blocks))
            else:
                assert all(len(r) == 2 + 2 * int(r[1]) for r in rows)
                cur.append(("V", np.array([int(r[0]) for r in rows], np.int32), [np.array(r[2:], np.int32).reshape(-1, 2) for r in rows]))
    assert not cur
    return rounds


class DescModel:
    """The naive model: one block per keyframe slot, one view list per point slot, the points' bad flags."""

    def __init__(self, n_points=0, n_keyframes=0):
        self.blocks = [np.zeros((0, 32), np.uint8) for _ in range(n_keyframes)]
        self.views = [np.zeros((0, 2), np.int32) for _ in range(n_points)]
        self.bad = np.zeros(n_points, np.uint8)

    def grow_points(self, n, bad=0):
        while len(self.views) < n:
            self.views.append(np.zeros((0, 2), np.int32))
        self.bad = np.concatenate([self.bad, np.full(n - len(self.bad), bad, np.uint8)])

    def set_blocks(self, kf_slots, blocks):
        for k, b in zip(kf_slots, blocks):
            while len(self.blocks) <= k:
                self.blocks.append(np.zeros((0, 32), np.uint8))
            self.blocks[k] = np.array(b, np.uint8).reshape(-1, 32)

    def set_views(self, slots, views):
        for p, v in zip(slots, views):
            self.views[p] = np.array(v, np.int32).reshape(-1, 2)

    def send(self, db, blocks=None, views=None):
        """Stages on the handle what it applies to itself."""
        if blocks is not None:
            db.set_keyframe_descriptors(*blocks)
            self.set_blocks(*blocks)
        if views is not None:
            db.set_point_views(*views)
            self.set_views(*views)

    def expected(self, slot, oracle):
        """(status, best, view, row) of one point: the rows gathered here, the winner by the oracle."""
        zero = (-1, (0, 0), np.zeros(32, np.uint8))
        if self.bad[slot]:
            return (BAD,) + zero
        rows, at = [], []
        for v, (kf, idx) in enumerate(self.views[slot]):
            blk = self.blocks[kf] if kf < len(self.blocks) else ()
            if len(blk) == 0:
                continue
            if idx >= len(blk):
                return (VIEW_OUT_OF_RANGE,) + zero
            rows.append(blk[idx])
            at.append(v)
        if not rows:
            return (NO_DESCRIPTORS,) + zero
        w = oracle.distinctive_descriptor(np.stack(rows))
        return UPDATED, at[w], tuple(int(x) for x in self.views[slot][at[w]]), rows[w]

    def check_query(self, db, slots, oracle):
        """db.distinctive_descriptors(slots) against expected(); returns the result."""
        slots = np.asarray(slots, np.int32).reshape(-1)
        got = db.distinctive_descriptors(slots)
        for q, s in enumerate(slots):
            st, best, view, row = self.expected(int(s), oracle)
            assert got["status"][q] == st and got["best"][q] == best, (q, int(s), int(got["status"][q]), st, int(got["best"][q]), best)
            assert tuple(got["best_view"][q]) == view and np.array_equal(got["desc"][q], row), (q, int(s))
        return got

    def check_exports(self, db):
        """Both exports against the model.  Returns ydorb_mapdb_desc_stats as it stood after the first export's sync."""
        views = db.export_views()
        stats = db.desc_stats()
        blocks = db.export_descriptors()
        assert len(views) == len(self.views) and len(blocks) >= len(self.blocks)
        for p, v in enumerate(views):
            assert np.array_equal(v, self.views[p]), p
        for k, b in enumerate(blocks):
            assert np.array_equal(b, self.blocks[k] if k < len(self.blocks) else np.zeros((0, 32), np.uint8)), k
        return stats


def median_ties(rows):
    """The medians of the sorted distance rows, from numpy alone: (least median, how many rows share it)."""
    rows = np.asarray(rows, np.uint8)
    d = np.unpackbits(rows[:, None, :] ^ rows[None, :, :], axis=2).sum(axis=2)
    med = np.sort(d, axis=1)[:, int(0.5 * len(rows))]
    return int(med.min()), int((med == med.min()).sum())
