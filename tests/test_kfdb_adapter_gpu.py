"""The C++ adapter include/ydorb/keyFrameDatabase.hpp EXECUTED on the GPU (tests/cpp_host/kfdb_run.cpp on stand-ins of KeyFrame /
Frame that carry BowVectors, covisibility lists and connected sets): the pointer-to-slot map, add / erase, touch() and the covisibility
push before a query, scoreAgainst, detectLoopCandidates, detectRelocalizationCandidates and its batch form; every result equals the
ctypes path (and so the CPU restatement) on the same scenario."""
import os
import struct
import subprocess

import numpy as np
import pytest

from kfdb_support import ROOT, SCENARIOS, compare, replay_gpu, replay_ref, scenario

pytestmark = pytest.mark.gpu
SRC = os.path.join(ROOT, "tests", "cpp_host", "kfdb_run.cpp")


def _build(tmp):
    exe = os.path.join(tmp, "kfdb_run")
    lib_dir = os.path.join(ROOT, "ydorbslam_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe, "-L" + lib_dir,
                           "-l:libydorb.so", "-Wl,-rpath," + lib_dir])
    return exe


def _vec(v):
    w, x = np.ascontiguousarray(v[0], "<i4"), np.ascontiguousarray(v[1], "<f8")
    return struct.pack("<i", len(w)) + w.tobytes() + x.tobytes()


def _ints(a):
    return np.asarray(a, "<i4").tobytes()


def _blob(ops):
    """The scenario in kfdb_run's format.  Neighbour and connected lists name key frames that are in the database at that point."""
    live, created, b = set(), 0, []
    for op in ops:
        if op[0] == "add":
            b.append(struct.pack("<ii", 0, len(op[1])) + b"".join(_vec(v) for v in op[1]))
            live |= set(range(created, created + len(op[1])))
            created += len(op[1])
        elif op[0] == "erase":
            b.append(struct.pack("<ii", 1, len(op[1])) + _ints(op[1]))
            live -= set(op[1])
        elif op[0] == "covis":
            b.append(struct.pack("<ii", 2, len(op[1])))
            for k, nb in zip(op[1], op[2]):
                nb = [m for m in nb if m in live]
                b.append(struct.pack("<ii", k, len(nb)) + _ints(nb))
        elif op[0] == "score":
            b.append(struct.pack("<i", 3) + _vec(op[1]) + struct.pack("<i", len(op[2])) + _ints(op[2]))
        elif op[0] == "reloc":
            b.append(struct.pack("<ii", 4, len(op[1])) + b"".join(_vec(q) for q in op[1]))
        elif op[0] == "loop":
            b.append(struct.pack("<ii", 5, len(op[1])))
            for q, c, m in zip(op[1], op[2], op[3]):
                c = [k for k in c if k in live]
                b.append(_vec(q) + struct.pack("<i", len(c)) + _ints(c) + struct.pack("<f", m))
    b.append(struct.pack("<i", -1))
    return b"".join(b)


def _read(path, ops):
    raw, at, out = open(path, "rb").read(), 0, []

    def get(dt, n=1):
        nonlocal at
        a = np.frombuffer(raw, dt, n, at)
        at += a.nbytes
        return a

    for op in ops:
        if op[0] == "score":
            out.append(("score", get("<f8", int(get("<i4")[0])).copy()))
        elif op[0] in ("reloc", "loop"):
            recs = []
            for _ in op[1]:
                n = int(get("<i4")[0])
                recs.append(dict(candidates=get("<i4", n).astype(np.int64), count=n, status=int(get("<i4")[0])))
            out.append((op[0], recs))
    assert at == len(raw)
    return out


@pytest.mark.parametrize("name", ["n1", "n37", "n3000"])
def test_adapter_equals_ctypes_and_restatement(tmp_path, name):
    n, seed = SCENARIOS[name]
    ops = scenario(n, seed, q_sizes=(1, 7))
    exe = _build(str(tmp_path))
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(inp, "wb").write(_blob(ops))
    subprocess.check_call([exe, inp, outp])
    got = _read(outp, ops)
    want = replay_gpu(ops, "L1_NORM")
    queries = 0
    for a, b in zip(want, got):
        assert a[0] == b[0]
        if a[0] == "score":
            assert np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
            continue
        for ra, rb in zip(a[1], b[1]):
            assert np.array_equal(ra["candidates"], rb["candidates"]), (ra["candidates"], rb["candidates"])
            if rb["status"] == -1:   # a batch reports only its last query's status
                rb["status"] = ra["status"]
            assert rb["status"] == ra["status"]
            queries += 1
    assert queries >= 32
    compare(replay_ref(ops, "L1_NORM"), got)   # the adapter's records carry no diagnostics; everything else against the restatement


def test_descriptors_to_candidate_to_search_by_bow():
    """End to end without a CPU algorithm step: descriptors -> ydorb_vocabulary_transform -> ydorb_kfdb_detect_reloc -> a candidate whose
    FeatureVector ydorb_search_by_bow accepts.  Six places (images), one key frame each; the lost frame is a shifted view of place 4.  The
    BowVector arrays transform returns go into add / detect_reloc as they are."""
    import ydorbslam_amd as y
    from helpers import shifted_pair
    from ydorbslam_amd.synth import synth_vocabulary
    voc = y.Vocabulary(synth_vocabulary(8, 4, seed=5))
    pairs = [shifted_pair(640, 480, 90 + s, 4, -2) for s in range(6)]
    ex = y.OrbExtractor(800, max_batch=12)
    feats = ex.extract_batch(np.stack([p[0] for p in pairs] + [p[1] for p in pairs]))
    bows = voc.transform([d for _, d in feats], 2)
    db = y.KeyFrameDatabase("L1_NORM")
    slots = db.add([(t[0], t[1]) for t in bows[:6]])
    lost = 6 + 4
    r = db.detect_reloc([(bows[lost][0], bows[lost][1])], diag=True)
    cand = r["candidates"][0].tolist()
    assert int(slots[4]) in cand, (cand, r["diag_words"])
    assert int(np.argmax(r["diag_score"])) == int(slots[4])           # the same place scores highest
    k = int(np.nonzero(slots == cand[cand.index(int(slots[4]))])[0][0])
    (ka, da), (kb, dbb) = feats[k], feats[lost]
    ta, tb = bows[k], bows[lost]
    fa = y.FeatureVector(ta[2].astype(np.uint32), ta[3], ta[4])
    fb = y.FeatureVector(tb[2].astype(np.uint32), tb[3], tb[4])
    n, out = y.OrbMatcher(0.75, True).search_by_bow(3, ka, da, np.ones(len(ka), np.uint8), fa, kb, dbb, None, fb)
    assert n > 20
    db.close()
