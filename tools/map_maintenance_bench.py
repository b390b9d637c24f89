"""Time of the three map-maintenance entries (ydorb_map_update_normal_depth, ydorb_map_covisibility, ydorb_map_keyframe_redundancy), host
to host at the C entry points on arrays prepared once, against the CPU restatement (tests/mapmaint_ref, one thread) on the same
flattened arrays in the same run, at two sizes:
  local  LocalMapping's: 31 keyframes of about 1500 map points each, 4-8 observers per point (about 7 750 points);
  map    a whole map: 5000 keyframes, 400 000 points, 4-8 observers from a window of 31 neighbouring keyframes.
Median wall time of the synchronous calls after warm-up with [min, max] beside it; the outputs of both sides are compared exactly
before timing.  Flat arrays flatter the CPU side against the reference's mutex-guarded containers, and the adapters' flattening is
outside both figures: --flatten runs tests/cpp_host/mapmaint_run.cpp on the local size and reports its host time per flattening.
The kernels alone: run this tool under `rocprofv3 --kernel-trace --stats -- python tools/map_maintenance_bench.py --size local` (and
`--size map`) and read the k_normal_depth / k_covisibility / k_redundancy rows; --kernel-ms NAME=MS turns such a figure into the
normal-and-depth kernel's achieved bytes per second.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mapmaint_support as S  # noqa: E402
import ydorbslam_amd as y  # noqa: E402
from ydorbslam_amd import map_maintenance as M  # noqa: E402

p = lambda a: a.ctypes.data_as(C.c_void_p)
SIZES = dict(local=(31, 7750, 31), map=(5000, 400000, 31))


def times(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return [round(float(v) * 1e3, 4) for v in (np.median(ts), min(ts), max(ts))]


def make_map(n_kf, n_points, window, seed=1):
    """Flat arrays of a map whose points are seen by 4-8 distinct keyframes out of `window` consecutive ones, in a shuffled order."""
    rng = np.random.default_rng(seed)
    m = rng.integers(4, 9, n_points)
    base = rng.integers(0, max(n_kf - window, 0) + 1, n_points)
    pick = np.argsort(rng.uniform(size=(n_points, window)), axis=1)[:, :8]          # 8 distinct offsets per point, shuffled
    keep = np.arange(8)[None, :] < m[:, None]
    obs_kf = (base[:, None] + pick)[keep].astype(np.int32)
    obs_start = np.concatenate([[0], np.cumsum(m)]).astype(np.int32)
    point_of = np.repeat(np.arange(n_points, dtype=np.int32), m)
    lvl_base = rng.integers(0, 8, n_points)
    level = np.clip(lvl_base[point_of] + rng.integers(-1, 2, len(obs_kf)), 0, 7).astype(np.uint8)
    stereo = rng.uniform(size=len(obs_kf)) < 0.5
    T = M.ObservationTable.from_arrays(n_kf, obs_start, obs_kf, level | np.where(stereo, 0x80, 0).astype(np.uint8),
                                       (rng.uniform(size=n_points) < 0.02).astype(np.uint8))
    by_kf = np.argsort(obs_kf, kind="stable")                                      # each keyframe's map-point vector
    kf_start = np.concatenate([[0], np.cumsum(np.bincount(obs_kf, minlength=n_kf))]).astype(np.int32)
    first = obs_start[:-1]
    return dict(T=T, pos=(rng.uniform(-6, 6, (n_points, 3)) + [0, 0, 12]).astype(np.float32), centre=rng.uniform(-4, 4, (n_kf, 3)).astype(np.float32),
                ref_kf=np.ascontiguousarray(obs_kf[first]), ref_level=np.ascontiguousarray(level[first]), kf_start=kf_start,
                kf_points=np.ascontiguousarray(point_of[by_kf]), kf_levels=np.ascontiguousarray(level[by_kf]), n_obs=len(obs_kf))


def bench_size(name, reps):
    n_kf, n_points, window = SIZES[name]
    L, R = y.lib(), S.ref()
    d = make_map(n_kf, n_points, window)
    T, sf = d["T"], S.scale_factors()
    out = dict(keyframes=n_kf, points=n_points, observations=d["n_obs"])

    def both(label, gpu_fn, ref_fn, make_args, outputs):
        a, b = make_args(), make_args()
        assert gpu_fn(*a) == 0, L.ydorb_last_error()
        assert ref_fn(*b) == 0
        for k in outputs:
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (label, k)
        out[label] = dict(gpu_ms=times(lambda: gpu_fn(*a), reps), cpu_ms=times(lambda: ref_fn(*b), max(3, reps // 3)))

    class Args(list):   # ctypes arguments that keep their numpy arrays reachable by position
        def __init__(self, items):
            super().__init__(items)
            self.c = [p(v) if isinstance(v, np.ndarray) else v for v in items]

        def __iter__(self):
            return iter(self.c)

    def nd_args():
        return Args([C.byref(T.struct), d["pos"], d["centre"], d["ref_kf"], d["ref_level"], sf, 8, 0, np.zeros((n_points, 3), np.float32),
                     np.zeros(n_points, np.float32), np.zeros(n_points, np.float32), np.zeros(n_points, np.uint8)])

    both("normal_depth", L.ydorb_map_update_normal_depth, R.mapref_update_normal_depth, nd_args, (8, 9, 10, 11))
    out["normal_depth"]["algorithmic_bytes"] = int(n_points * (8 + 12 + 4 + 1 + 1 + 21) + d["n_obs"] * (4 + 12))

    def lists(kfs):
        start = np.concatenate([[0], np.cumsum(d["kf_start"][kfs + 1] - d["kf_start"][kfs])]).astype(np.int32)
        idx = np.concatenate([d["kf_points"][d["kf_start"][k]:d["kf_start"][k + 1]] for k in kfs]).astype(np.int32)
        own = np.concatenate([d["kf_levels"][d["kf_start"][k]:d["kf_start"][k + 1]] for k in kfs]).astype(np.uint8)
        return start, np.ascontiguousarray(idx), np.ascontiguousarray(own)

    for label, q in (("covisibility_1", np.array([n_kf // 2], np.int32)), ("covisibility_all", np.arange(n_kf, dtype=np.int32))):
        start, idx, _ = lists(q)
        span = T.span_lengths()
        caps = [min(n_kf - 1, int(span[idx[start[i]:start[i + 1]]].sum())) for i in range(len(q))]
        out_start = np.concatenate([[0], np.cumsum(caps)]).astype(np.int32)

        def cv_args():
            return Args([C.byref(T.struct), q, len(q), start, idx, out_start, 0, np.full(max(int(out_start[-1]), 1), -1, np.int32),
                         np.full(max(int(out_start[-1]), 1), -1, np.int32), np.zeros(len(q), np.int32), np.zeros(len(q), np.uint8)])

        both(label, L.ydorb_map_covisibility, R.mapref_covisibility, cv_args, (7, 8, 9, 10))
        out[label]["queries"], out[label]["list_entries"] = len(q), int(start[-1])

    cand = np.arange(1, n_kf, dtype=np.int32)
    start, idx, own = lists(cand)
    removed = np.zeros(n_kf, np.uint8)
    removed[cand[::7]] = 1
    for label, rem in (("redundancy", None), ("redundancy_masked", removed)):
        def rd_args():
            return Args([C.byref(T.struct), cand, len(cand), start, idx, own, rem, 3, 0, np.zeros(len(cand), np.int32), np.zeros(len(cand), np.int32),
                         np.zeros(len(cand), np.uint8)])

        both(label, L.ydorb_map_keyframe_redundancy, R.mapref_keyframe_redundancy, rd_args, (9, 10, 11))
        out[label]["candidates"], out[label]["list_entries"] = len(cand), int(start[-1])
    return out


def flatten_times():
    """Host time of the adapters' three flattenings on stand-ins at the local size (31 keyframes, 7 750 points)."""
    m = S.random_map(5, 31, 7750, 4, 8, level_spread=1)
    scene = S.adapter_scene(m, 8.0, seed=2)
    tmp = tempfile.mkdtemp(prefix="mmbench")
    exe = S.build_adapter_exe(os.path.join(tmp, "mapmaint_run"))
    runs = [S.run_adapters(exe, tmp, scene, 0, list(range(31)), [15], S.scale_factors())["flatten_us"] for _ in range(5)]
    return {k: round(float(np.median([r[k] for r in runs])) / 1e3, 4) for k in runs[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", choices=["local", "map", "both"], default="both")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--flatten", action="store_true")
    ap.add_argument("--kernel-ms", action="append", default=[], help="SIZE=MS: k_normal_depth's time from a kernel trace, for the bytes-per-second figure")
    a = ap.parse_args()
    res = {}
    for name in (["local", "map"] if a.size == "both" else [a.size]):
        res[name] = bench_size(name, a.reps)
    for kv in a.kernel_ms:
        name, ms = kv.split("=")
        if name in res:
            nd = res[name]["normal_depth"]
            nd["kernel_ms"] = float(ms)
            nd["kernel_GB_per_s"] = round(nd["algorithmic_bytes"] / (float(ms) * 1e-3) / 1e9, 1)
    if a.flatten:
        res["flatten_ms_local"] = flatten_times()
    M.release()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
