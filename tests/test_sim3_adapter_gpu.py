"""The C++ adapters include/ydorb/sim3Solver.hpp and optimizeSim3Impl EXECUTED on the GPU (tests/cpp_host/sim3_run.cpp on stand-ins of
KeyFrame / MapPoint that carry data): the constructor's predicates, float camera-frame transforms, maxError and indices1, the RandomInt
draw from rand(), and the results equal the ctypes path on the same flat problem."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from sim3_support import ROOT, rot

pytestmark = pytest.mark.gpu
SRC = os.path.join(ROOT, "tests", "cpp_host", "sim3_run.cpp")
K = (520.0, 515.0, 320.0, 240.0)
SIG2 = (np.float32(1.2) ** (2 * np.arange(8))).astype(np.float32)


def _build(tmp):
    exe = os.path.join(tmp, "sim3_run")
    lib_dir = os.path.join(ROOT, "ydorbslam_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpu_harness", "mockrt"),
                           "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe, "-L" + lib_dir, "-l:libydorb.so", "-Wl,-rpath," + lib_dir])
    return exe


def _scene(seed, nMP=150, outliers=0.3):
    """World points seen by two keyframes; matched12[i] is the true point for most keypoints of KF1, another point for outliers, none
    for some; a few points are bad or not indexed in KF2."""
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.uniform(-2, 2, nMP), rng.uniform(-1.5, 1.5, nMP), rng.uniform(3, 9, nMP)], axis=1).astype(np.float32)
    T = [np.hstack([np.eye(3), np.zeros((3, 1))]).astype(np.float32),
         np.hstack([rot(rng, 0.1), rng.uniform(-0.3, 0.3, (3, 1))]).astype(np.float32)]
    bad = rng.uniform(size=nMP) < 0.05
    nKP1, nKP2 = nMP + 10, nMP
    idx1 = np.arange(nMP, dtype=np.int32)
    idx2 = rng.permutation(nMP).astype(np.int32)
    idx2[rng.uniform(size=nMP) < 0.05] = -1
    kps = []
    for k, (n, idx) in enumerate(((nKP1, idx1), (nKP2, idx2))):
        xy = rng.uniform(0, 600, (n, 2)).astype(np.float32)
        Xc = pos @ T[k][:, :3].T + T[k][:, 3]
        uv = np.stack([K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]], axis=1) + rng.normal(0, 0.5, (nMP, 2))
        ok = idx >= 0
        xy[idx[ok]] = uv[ok]
        kps.append((xy, rng.integers(0, 8, n).astype(np.int32)))
    mps1 = np.full(nKP1, -1, np.int32)
    mps1[idx1] = np.arange(nMP)
    matched = mps1.copy()
    out = rng.uniform(size=nKP1) < outliers
    matched[out] = rng.integers(0, nMP, out.sum())
    matched[rng.uniform(size=nKP1) < 0.05] = -1
    return dict(pos=pos, T=T, bad=bad, idx1=idx1, idx2=idx2, kps=kps, mps1=mps1, matched=matched)


def _blob(s):
    b = [np.array([len(s["pos"]), len(s["kps"][0][0]), len(s["kps"][1][0])], np.int32).tobytes(), np.array(K, np.float32).tobytes()]
    for k in range(2):
        b += [s["T"][k][:, :3].astype(np.float32).tobytes(), s["T"][k][:, 3].astype(np.float32).tobytes(), SIG2.tobytes(),
              (np.float32(1) / SIG2).astype(np.float32).tobytes()]
        xy, octv = s["kps"][k]
        rec = np.zeros(len(xy), [("x", "<f4"), ("y", "<f4"), ("o", "<i4")])
        rec["x"], rec["y"], rec["o"] = xy[:, 0], xy[:, 1], octv
        b.append(rec.tobytes())
    rec = np.zeros(len(s["pos"]), [("p", "<f4", 3), ("bad", "<i4"), ("i1", "<i4"), ("i2", "<i4")])
    rec["p"], rec["bad"], rec["i1"], rec["i2"] = s["pos"], s["bad"], s["idx1"], s["idx2"]
    b += [rec.tobytes(), s["mps1"].tobytes(), s["matched"].tobytes()]
    return b"".join(b)


def _flat(s):
    """The constructor restated: kept pairs, their float camera-frame points, images and maxError."""
    from ydorbslam_amd.sim3 import camera_points, camera_to_image
    keep = [i for i in range(len(s["matched"])) if s["matched"][i] >= 0 and s["mps1"][i] >= 0 and not s["bad"][s["mps1"][i]]
            and not s["bad"][s["matched"][i]] and s["idx1"][s["mps1"][i]] >= 0 and s["idx2"][s["matched"][i]] >= 0]
    m1, m2 = s["mps1"][keep], s["matched"][keep]
    X1, X2 = camera_points(s["pos"][m1], s["T"][0]), camera_points(s["pos"][m2], s["T"][1])
    me = lambda k, idx: np.floor(9.210 * SIG2[s["kps"][k][1][idx]].astype(np.float64)).astype(np.float32)
    return dict(indices1=np.array(keep, np.int32), X1=X1, X2=X2, P1=camera_to_image(X1, K), P2=camera_to_image(X2, K),
                max_err1=me(0, s["idx1"][m1]), max_err2=me(1, s["idx2"][m2]), m1=m1, m2=m2)


def _read(path, spec):
    raw = open(path, "rb").read()
    out, at = {}, 0
    for name, dt, n in spec:
        n = n(out) if callable(n) else n
        a = np.frombuffer(raw, dt, n, at)
        at += a.nbytes
        out[name] = a
    assert at == len(raw)
    return out


@pytest.mark.parametrize("fix_scale", [1, 0])
def test_sim3_solver_adapter_equals_ctypes(tmp_path, fix_scale):
    from ydorbslam_amd.sim3 import ransac, ransac_iterations
    exe = _build(str(tmp_path))
    s = _scene(5 + fix_scale)
    seed, min_inl, max_its = 1234, 20, 300
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(inp, "wb").write(_blob(s) + np.array([seed, min_inl, max_its, fix_scale], np.int32).tobytes())
    subprocess.check_call([exe, "ransac", inp, outp])
    nKP1 = len(s["matched"])
    N = int(np.frombuffer(open(outp, "rb").read(4), np.int32)[0])
    g = _read(outp, [("N", "<i4", 1), ("indices1", "<i4", N), ("X1", "<f4", 3 * N), ("X2", "<f4", 3 * N), ("P1", "<f4", 2 * N),
                     ("P2", "<f4", 2 * N), ("me1", "<f4", N), ("me2", "<f4", N), ("maxIts", "<i4", 1), ("calls", "<i4", 1),
                     ("nTri", "<i4", 1), ("tri", "<i4", lambda o: int(o["nTri"][0])), ("ret", "<i4", 1), ("noMore", "<i4", 1),
                     ("nInl", "<i4", 1), ("inl", "u1", nKP1), ("T", "<f4", 16), ("R", "<f4", 9), ("t", "<f4", 3), ("s", "<f4", 1)])
    f = _flat(s)
    # the constructor: predicates, indices1, float transforms, images, size_t maxError
    assert np.array_equal(g["indices1"], f["indices1"])
    for a, b in (("X1", "X1"), ("X2", "X2"), ("P1", "P1"), ("P2", "P2"), ("me1", "max_err1"), ("me2", "max_err2")):
        assert np.array_equal(g[a].view(np.uint32), np.ascontiguousarray(f[b]).reshape(-1).view(np.uint32)), a
    assert g["maxIts"][0] == ransac_iterations(N, 0.99, min_inl, max_its)
    # the draw: RandomInt over rand() seeded as the harness seeded it, 5 triples per iterate(5) or what maxIts leaves
    # glibc's stream for the seed, taken before this process makes GPU calls of its own (the runtime may draw from rand() too)
    libc = C.CDLL(None)
    libc.rand.restype = C.c_int
    libc.srand(C.c_uint(seed))
    stream = iter([libc.rand() for _ in range(3 * 5 * 200)])
    rand_int = lambda lo, hi: int((next(stream) / (2147483647 + 1.0)) * (hi - lo + 1)) + lo
    # the ctypes path on the same flat problem, call by call with the same triples
    prob = dict(X1=f["X1"], X2=f["X2"], P1=f["P1"], P2=f["P2"], max_err1=f["max_err1"], max_err2=f["max_err2"], K1=K, K2=K,
                fix_scale=bool(fix_scale), min_inliers=min_inl, max_its=int(g["maxIts"][0]), next_hyp=0, best_inliers=0,
                best_T12=np.zeros(13, np.float32))
    drawn, calls = [], 0
    while True:
        calls += 1
        tri = []
        for _ in range(max(0, min(5, prob["max_its"] - prob["next_hyp"]))):
            avail = list(range(N))
            for _ in range(3):
                r = rand_int(0, len(avail) - 1)
                tri.append(avail[r]); avail[r] = avail[-1]; avail.pop()
        drawn += tri
        r = ransac([dict(prob, triples=np.array(tri, np.int32).reshape(-1, 3))], chunk=5)[0]
        prob.update(next_hyp=r["next_hyp"], best_inliers=r["best_inliers"], best_T12=r["best_T12"])
        if r["ret_hyp"] >= 0 or r["no_more"]:
            break
    assert np.array_equal(g["tri"], np.array(drawn, np.int32))
    assert g["calls"][0] == calls and g["ret"][0] == (r["ret_hyp"] >= 0) and g["noMore"][0] == r["no_more"]
    assert g["ret"][0] == 1   # the scene's true Sim3 is found
    inl = np.zeros(nKP1, bool)
    inl[f["indices1"][r["inliers"]]] = True
    assert np.array_equal(g["inl"].astype(bool), inl) and g["nInl"][0] == r["inliers"].sum()
    b = r["best_T12"]
    T = np.zeros(16, np.float32)
    T.reshape(4, 4)[:3, :3] = (b[12] * b[:9]).reshape(3, 3)
    T.reshape(4, 4)[:3, 3] = b[9:12]
    T[15] = 1
    assert np.array_equal(g["T"].view(np.uint32), T.view(np.uint32))
    assert np.array_equal(np.concatenate([g["R"], g["t"], g["s"]]).view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("fix_scale", [1, 0])
def test_optimize_sim3_adapter_equals_ctypes(tmp_path, fix_scale):
    from ydorbslam_amd.sim3 import optimize_sim3
    from sim3_support import quat_xyzw
    exe = _build(str(tmp_path))
    s = _scene(11 + fix_scale, outliers=0.15)
    T1, T2 = s["T"][0].astype(np.float64), s["T"][1].astype(np.float64)
    R12 = T1[:, :3] @ T2[:, :3].T                      # S12 maps KF2's camera frame to KF1's
    t12 = T1[:, 3] - R12 @ T2[:, 3]
    S12 = np.concatenate([quat_xyzw(rot(np.random.default_rng(3), 0.01) @ R12), t12 + 0.01, [1.0]])
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(inp, "wb").write(_blob(s) + S12.tobytes() + np.array([10.0], np.float32).tobytes() + np.array([fix_scale], np.int32).tobytes())
    subprocess.check_call([exe, "opt", inp, outp])
    nKP1 = len(s["matched"])
    g = _read(outp, [("n", "<i4", 1), ("S12", "<f8", 8), ("matches", "<i4", nKP1)])
    # optimizeSim3's pair predicates: both points set and not bad, KF2's index >= 0 (KF1's keypoint is the match index itself)
    keep = [i for i in range(nKP1) if s["matched"][i] >= 0 and s["mps1"][i] >= 0 and not s["bad"][s["mps1"][i]]
            and not s["bad"][s["matched"][i]] and s["idx2"][s["matched"][i]] >= 0]
    from ydorbslam_amd.sim3 import camera_points
    m1, m2 = s["mps1"][keep], s["matched"][keep]
    i2 = s["idx2"][m2]
    prob = dict(X1c=camera_points(s["pos"][m1], s["T"][0]).astype(np.float64), X2c=camera_points(s["pos"][m2], s["T"][1]).astype(np.float64),
                obs1=s["kps"][0][0][keep].astype(np.float64), obs2=s["kps"][1][0][i2].astype(np.float64),
                inv_sigma2_1=(np.float32(1) / SIG2)[s["kps"][0][1][keep]].astype(np.float64),
                inv_sigma2_2=(np.float32(1) / SIG2)[s["kps"][1][1][i2]].astype(np.float64),
                K1=np.array(K, np.float32).astype(np.float64), K2=np.array(K, np.float32).astype(np.float64), S12=S12, fix_scale=bool(fix_scale))
    r = optimize_sim3([prob])[0]
    assert g["n"][0] == r["n_in"] > 100
    assert np.array_equal(g["S12"], r["S12"])
    want = s["matched"].copy()
    want[np.array(keep)[r["outlier"]]] = -1
    assert np.array_equal(g["matches"], want)
