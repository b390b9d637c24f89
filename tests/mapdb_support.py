"""Test support of the resident map table: builds tests/cpu_harness/mapdb_host_check.cpp without sanitizers to obtain its seeded
operation sequence and counter trace (the GPU test replays both through the real handle), keeps the naive model that sequence is
checked against (per-slot records, re-flattened from scratch), and loads mapmaint_support's tables into a handle."""
import os
import subprocess

import numpy as np

import mapmaint_support as S
from mapmaint_support import ROOT

CHECK_SRC = os.path.join(ROOT, "tests", "cpu_harness", "mapdb_host_check.cpp")
TRACE_FIELDS = ("round", "n_points", "n_keyframes", "n_observations", "pool_used", "pool_capacity", "repacks_kept", "repacks_grown",
                "point_table_growths", "keyframe_table_growths", "point_capacity", "keyframe_capacity", "last_sync_bytes", "last_sync_records")
SEQUENCE_CAPACITIES = (640, 48, 4096)   # the Db of the check program's sequence: points, keyframes, observations


def parse_trace(lines):
    out = []
    for ln in lines:
        w = ln.split()
        assert w[0] == "trace" and len(w) == 1 + len(TRACE_FIELDS), ln
        out.append(dict(zip(TRACE_FIELDS, map(int, w[1:]))))
    return out


def _f32(words):
    return np.array([int(w) for w in words], np.int32).view(np.float32)


def check_ops(src, tmp):
    """Builds a check program of tests/cpu_harness without sanitizers, runs it and returns the lines of the operations file it wrote."""
    exe, ops = os.path.join(tmp, os.path.splitext(os.path.basename(src))[0]), os.path.join(tmp, "ops.txt")
    subprocess.check_call(["g++", "-std=c++17", "-O1", src, "-o", exe])
    subprocess.run([exe, ops], stdout=subprocess.DEVNULL, check=True)
    return open(ops).read().splitlines()


def sequence(tmp):
    """Runs the check program and returns its operations, one list per round: ("C", slots, centre), ("P", slots, observers, levels, bad,
    ref_kf, ref_level, pos), ("X", slots, pos), each round closed by ("S", trace)."""
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
        if w[0] in "CX":
            cur.append((w[0], slots, np.array([_f32(r[1:4]) for r in rows], np.float32).reshape(-1, 3)))
        else:
            lens = [int(r[7]) for r in rows]
            cur.append(("P", slots, [np.array(r[8:8 + m], np.int32) for r, m in zip(rows, lens)],
                        [np.array(r[8 + m:8 + 2 * m], np.uint8) for r, m in zip(rows, lens)], np.array([int(r[1]) for r in rows], np.uint8),
                        np.array([int(r[2]) for r in rows], np.int32), np.array([int(r[3]) for r in rows], np.uint8),
                        np.array([_f32(r[4:7]) for r in rows], np.float32).reshape(-1, 3)))
    assert not cur
    return rounds


class Model:
    """The naive model: per-slot records, flattened from scratch on demand.  A slot never set is bad with no observations."""

    def __init__(self):
        self.obs, self.lev, self.bad, self.ref_kf, self.ref_level, self.pos, self.centre = [], [], [], [], [], [], np.zeros((0, 3), np.float32)

    def _grow(self, n):
        while len(self.obs) < n:
            self.obs.append(np.zeros(0, np.int32)); self.lev.append(np.zeros(0, np.uint8)); self.bad.append(1); self.ref_kf.append(0)
            self.ref_level.append(0); self.pos.append(np.zeros(3, np.float32))

    def apply(self, op):
        if op[0] == "C":
            top = int(op[1].max()) + 1
            if top > len(self.centre):
                self.centre = np.concatenate([self.centre, np.zeros((top - len(self.centre), 3), np.float32)])
            for s, c in zip(op[1], op[2]):
                self.centre[s] = c
        elif op[0] == "X":
            for s, p in zip(op[1], op[2]):
                self.pos[s] = p.copy()
        else:
            _, slots, obs, lev, bad, ref_kf, ref_level, pos = op
            self._grow(int(slots.max()) + 1)
            for i, s in enumerate(slots):
                self.obs[s], self.lev[s], self.bad[s], self.ref_kf[s], self.ref_level[s], self.pos[s] = obs[i], lev[i], int(bad[i]), int(ref_kf[i]), int(ref_level[i]), pos[i].copy()

    def send(self, db, op):
        if op[0] == "C":
            db.set_centres(op[1], op[2])
        elif op[0] == "X":
            db.set_positions(op[1], op[2])
        else:
            db.set_points(*op[1:])

    def flat(self):
        """dict(table, pos, centre, ref_kf, ref_level, kf_points, kf_levels) of the model as it stands."""
        from ydorbslam_amd.map_maintenance import ObservationTable, _csr
        start, kf = _csr(self.obs, np.int32)
        _, lv = _csr(self.lev, np.uint8)
        T = ObservationTable.from_arrays(len(self.centre), start, kf, lv, np.array(self.bad, np.uint8))
        kf_points, kf_levels = [[] for _ in self.centre], [[] for _ in self.centre]
        for p, (o, l) in enumerate(zip(self.obs, self.lev)):
            for k, v in zip(o, l):
                kf_points[k].append(p)
                kf_levels[k].append(int(v) & 0x7f)
        return dict(table=T, pos=np.array(self.pos, np.float32).reshape(-1, 3), centre=self.centre.copy(), ref_kf=np.array(self.ref_kf, np.int32),
                    ref_level=np.array(self.ref_level, np.uint8), kf_points=[np.array(a, np.int32) for a in kf_points],
                    kf_levels=[np.array(a, np.uint8) for a in kf_levels])


def same_export(got, want):
    """The read-back table against a flat one: every integer, byte and float bit pattern."""
    G, W = got["table"], want["table"]
    assert (G.n_points, G.n_keyframes) == (W.n_points, W.n_keyframes)
    for k in ("obs_start", "obs_kf", "obs_level", "bad"):
        assert np.array_equal(getattr(G, k), getattr(W, k)), k
    for k in ("ref_kf", "ref_level"):
        assert np.array_equal(got[k], np.asarray(want[k], got[k].dtype)), k
    for k in ("pos", "centre"):
        assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint32), np.ascontiguousarray(want[k], np.float32).view(np.uint32)), k


def split_levels(table):
    """Per point the observers and the level bytes of a flat table."""
    st = table.obs_start
    return ([table.obs_kf[st[p]:st[p + 1]] for p in range(table.n_points)], [table.obs_level[st[p]:st[p + 1]] for p in range(table.n_points)])


def load(db, m, order=None, calls=1):
    """A mapmaint_support map (or Model.flat()) into `db`: the centres, then the points in `order` over `calls` set_points calls."""
    T = m["table"]
    db.set_centres(np.arange(T.n_keyframes), m["centre"])
    obs, lev = split_levels(T)
    order = np.arange(T.n_points) if order is None else np.asarray(order)
    for part in np.array_split(order, calls):
        db.set_points(part, [obs[p] for p in part], [lev[p] for p in part], T.bad[part], np.asarray(m["ref_kf"])[part], np.asarray(m["ref_level"])[part],
                      np.asarray(m["pos"], np.float32)[part])


def three_queries_equal_the_restatement(db, m, sf=None):
    """Normals of every slot, covisibility of every keyframe and the redundancy of every keyframe but slot 0, resident against the CPU
    restatement on the flat table `m`."""
    sf = S.scale_factors() if sf is None else sf
    T = m["table"]
    S.same_normal_depth(db.update_normal_depth(np.arange(T.n_points), sf), S.ref_update_normal_depth(T, m["pos"], m["centre"], m["ref_kf"], m["ref_level"], sf))
    q = np.arange(T.n_keyframes, dtype=np.int32)
    S.same_covisibility(db.covisibility(q, m["kf_points"]), S.ref_covisibility(T, q, m["kf_points"]))
    cand, lists, own = S.candidates(m)
    S.same_redundancy(db.keyframe_redundancy(cand, lists, own), S.ref_keyframe_redundancy(T, cand, lists, own))


# ------------------------------------------------------------------------------------------------------------ adapter program
def build_mirror_exe(out):
    lib_dir = os.path.join(ROOT, "ydorbslam_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpu_harness", "mockrt"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp_host", "mapdb_run.cpp"), "-o", out,
                           "-L" + lib_dir, "-l:libydorb.so", "-Wl,-rpath," + lib_dir])
    return out


def run_mirror(exe, tmp, scene, current, covisible, queries, sf, reps=0):
    """Runs tests/cpp_host/mapdb_run.cpp on a mapmaint_support.adapter_scene.  Returns {name: int}, and {"time_...": [median, min, max]}."""
    inp = os.path.join(tmp, "in.bin")
    open(inp, "wb").write(S.adapter_blob(scene, current, covisible, queries, sf))
    r = subprocess.run([exe, inp] + ([str(reps)] if reps else []), stdout=subprocess.PIPE, text=True, check=True)
    out = {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        out[w[0]] = [float(v) for v in w[1:]] if w[0].startswith("time_") else int(w[1])
    return out
