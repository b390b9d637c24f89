"""Throughput of the key-frame database: ydorb_kfdb_detect_reloc queries/s at N in {1 k, 10 k, 50 k} key frames of ~1000 words and
Q in {1, 64} queries per call, host to host, against the test restatement (tests/kfdb_ref/kfdb_ref.cpp, inverted file, one CPU
thread) on the same data in the same run; two queries are checked for equal candidates first.  Each figure: 5 repeats after warm-up,
median and min-max spread.  Also the bytes of rows a call reads (12 B per stored word and query) over its time, to set against HBM
bandwidth.  Prints one JSON line.
--sizes 1000,10000 limits the N values."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from kfdb_support import RefDatabase, World  # noqa: E402
from ydorbslam_amd.kfdb import KeyFrameDatabase  # noqa: E402


def times(fn, reps=5):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    sizes = (1000, 10000, 50000)
    if "--sizes" in sys.argv:
        sizes = tuple(int(s) for s in sys.argv[sys.argv.index("--sizes") + 1].split(","))
    out = {"metric": "kfdb_reloc_queries_per_s", "reloc": {}}
    for N in sizes:
        W = World(N, N, vocab=1000000, words=(800, 1200))
        words = int(sum(len(w) for w, _ in W.vectors))
        covis = [W.covisibility(k) for k in range(N)]   # drawn once: both sides get the same lists
        db = KeyFrameDatabase("L1_NORM")
        slots = db.add(W.vectors)
        assert np.array_equal(slots, np.arange(N))      # a fresh database hands out slots in add order = the restatement's ids
        db.set_covisibility(slots, covis)
        rdb = RefDatabase("L1_NORM")
        for v in W.vectors:
            rdb.add(v)
        for k in range(N):
            rdb.set_covisibility(k, covis[k])
        qs = [W.query(2) for _ in range(64)]
        # the timed data gives the same answer on both sides (and leaves both with the same relocalisation scores)
        for q in qs[:2]:
            want, got = rdb.detect(q, diag=False), db.detect_reloc([q])
            assert np.array_equal(want["candidates"], got["candidates"][0]) and want["status"] == int(got["status"][0])
        cpu, cpu_lo, cpu_hi = times(lambda: [rdb.detect(q, diag=False) for q in qs[:8]], 3)
        cpu, cpu_lo, cpu_hi = cpu / 8, cpu_lo / 8, cpu_hi / 8
        for Q in (1, 64):
            db.detect_reloc(qs[:Q], cand_cap=64)   # warm-up: scratch allocation, code-object load
            g, lo, hi = times(lambda: db.detect_reloc(qs[:Q], cand_cap=64))
            out["reloc"]["N%d_Q%d" % (N, Q)] = {
                "gpu_ms_per_call": round(g * 1e3, 3), "gpu_ms_min_max": [round(lo * 1e3, 3), round(hi * 1e3, 3)],
                "gpu_queries_per_s": round(Q / g, 1), "cpu_queries_per_s": round(1 / cpu, 1),
                "cpu_ms_min_max": [round(cpu_lo * 1e3, 3), round(cpu_hi * 1e3, 3)],
                "row_bytes_per_query": 12 * words, "row_gbytes_per_s": round(12 * words * Q / g / 1e9, 1)}
        db.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
