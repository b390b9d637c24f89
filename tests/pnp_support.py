"""Test support of the relocalisation EPnP RANSAC: builds the CPU restatement tests/pnp_ref/pnp_ref.cpp with oracle/Makefile's
compiler flags and makes synthetic relocalisation problems with a known camera pose."""
import ctypes as C
import os
import re
import shlex
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "pnp_ref", "pnp_ref.cpp")
_REF = None

K_VGA = (520.0, 518.0, 320.0, 240.0)   # 640 x 480


def _flags():
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return shlex.split(re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1))


def ref():
    global _REF
    if _REF is None:
        out = os.path.join(tempfile.mkdtemp(prefix="pnpref"), "libpnpref.so")
        subprocess.check_call(["g++", *_flags(), "-shared", "-o", out, SRC, "-lm"])
        L = C.CDLL(out)
        L.pnpref_params.argtypes = [C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
        L.pnpref_ransac.argtypes = [C.c_int] + [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7
        for f in ("pnpref_eig_sym", "pnpref_svd", "pnpref_lstsq", "pnpref_qr_solve", "pnpref_epnp"):
            getattr(L, f).restype = None
        _REF = L
    return _REF


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _c(a, dt):
    return np.ascontiguousarray(a, dt)


def ref_params(N, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4):
    out = np.zeros(2, np.int32)
    eps = np.zeros(1, np.float32)
    ref().pnpref_params(N, probability, min_inliers, max_iterations, min_set, epsilon, _p(out), _p(eps))
    return int(out[0]), int(out[1]), float(eps[0])


def ref_eig_sym(A):
    A = _c(A, np.float64)
    n = len(A)
    d, ut = np.zeros(n), np.zeros((n, n))
    ref().pnpref_eig_sym(n, _p(A), _p(d), _p(ut))
    return d, ut


def ref_svd(A):
    A = _c(A, np.float64)
    m, k = A.shape
    w, U, V = np.zeros(k), np.zeros((m, k)), np.zeros((k, k))
    ref().pnpref_svd(m, k, _p(A), _p(w), _p(U), _p(V))
    return w, U, V


def ref_lstsq(A, b):
    A, b = _c(A, np.float64), _c(b, np.float64)
    x = np.zeros(A.shape[1])
    ref().pnpref_lstsq(A.shape[0], A.shape[1], _p(A), _p(b), _p(x))
    return x


def ref_epnp(Xw, P2D, K, idx=None):
    Xw, P2D = _c(Xw, np.float32).reshape(-1, 3), _c(P2D, np.float32).reshape(-1, 2)
    idx = _c(np.arange(len(Xw)) if idx is None else idx, np.int32)
    out = np.zeros(13)
    ref().pnpref_epnp(_p(Xw), _p(P2D), _p(_c(K, np.float32)), _p(idx), len(idx), _p(out))
    return out[:9].reshape(3, 3), out[9:12], out[12]


def ref_ransac(prob, chunk):
    """The oracle's iterate(chunk) sequence on a problem dict of ydorbslam_amd.pnp.ransac."""
    Xw, P2D = _c(prob["Xw"], np.float32).reshape(-1, 3), _c(prob["P2D"], np.float32).reshape(-1, 2)
    me = _c(prob["max_err"], np.float32).reshape(-1)
    N = len(Xw)
    quads = _c(np.asarray(prob["quads"], np.int32).reshape(-1, 4), np.int32)
    state = np.array([prob.get("next_hyp", 0), prob.get("best_inliers", 0)], np.int32)
    bmask = np.zeros(max(N, 1), np.uint8)
    if prob.get("best_mask") is not None:
        bmask[:N] = np.asarray(prob["best_mask"], bool)
    btcw = np.array(prob.get("best_Tcw", np.zeros(12)), np.float32).reshape(12)
    out = np.zeros(5, np.int32)
    tcw = np.zeros(12, np.float32)
    mask = np.zeros(max(N, 1), np.uint8)
    hyp = np.zeros(max(len(quads), 1), np.int32)
    ref().pnpref_ransac(N, _p(Xw), _p(P2D), _p(me), _p(_c(prob["K"], np.float32)), int(prob["min_inliers"]), int(prob["max_its"]),
                        int(bool(prob.get("loop_or", True))), _p(quads), len(quads), int(chunk), _p(state), _p(bmask), _p(btcw),
                        _p(out), _p(tcw), _p(mask), _p(hyp))
    return dict(ret_hyp=int(out[0]), ret_how=int(out[1]), no_more=bool(out[2]), n_calls=int(out[3]), n_inliers=int(out[4]), Tcw=tcw,
                inliers=mask[:N].astype(bool), hyp_inliers=hyp[:len(quads)].copy(), next_hyp=int(state[0]), best_inliers=int(state[1]),
                best_mask=bmask[:N].astype(bool), best_Tcw=btcw)


# ------------------------------------------------------------------------------------------------------------ synthetic problems
def rot(rng, max_angle):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = rng.uniform(-max_angle, max_angle)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def project(Xc, K):
    return np.stack([K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]], axis=1)


def synth_scene(N, seed, planar=False, K=K_VGA):
    """N points in front of a camera with a random Tcw, imaged noise-free through K (float64)."""
    rng = np.random.default_rng(seed)
    R = rot(rng, np.pi)
    t = rng.uniform(-1, 1, 3)
    u = rng.uniform(20, 620, N)
    v = rng.uniform(20, 460, N)
    if planar:   # points on a tilted plane in the camera frame
        n = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 1.0])
        rays = np.stack([(u - K[2]) / K[0], (v - K[3]) / K[1], np.ones(N)], axis=1)
        z = 5.0 / (rays @ n)
        Xc = rays * z[:, None]
    else:
        z = rng.uniform(2, 10, N)
        Xc = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], axis=1)
    Xw = (Xc - t) @ R   # R^T (Xc - t)
    return Xw, project(Xc, K), R, t


def synth_problem(N, seed, outliers=0.0, noise=0.5, min_inliers=10, epsilon=0.5, n_hyp=None, loop_or=True, K=K_VGA, max_its=None):
    """A relocalisation problem: N map points against a frame with a known Tcw, octaves 0..7 (sigma^2 = 1.2^(2 octave)), pixel noise and
    a fraction of outlier matches; quads drawn by the reference's procedure.  Returns (problem dict of ydorbslam_amd.pnp.ransac, R, t)."""
    from ydorbslam_amd.pnp import RandGen, draw_quads, ransac_parameters, sequence_length
    rng = np.random.default_rng(seed + 7919)
    Xw, uv, R, t = synth_scene(N, seed, K=K)
    octave = rng.integers(0, 8, N)
    sigma2 = (np.float32(1.2) ** (2 * octave)).astype(np.float32)
    uv = uv + rng.normal(0, noise, (N, 2)) * np.sqrt(sigma2)[:, None]
    nb = int(round(outliers * N))
    if nb:
        bad = rng.choice(N, nb, replace=False)
        uv[bad] = np.stack([rng.uniform(0, 640, nb), rng.uniform(0, 480, nb)], axis=1)
    n_min, its, _ = ransac_parameters(N, 0.99, min_inliers, 300, 4, epsilon)
    if max_its is not None:
        its = max_its
    H = sequence_length(N, n_min, its, 0, 5, loop_or) if n_hyp is None else n_hyp
    quads = draw_quads(N, H, RandGen(seed)) if N >= 4 else np.zeros((0, 4), np.int32)
    prob = dict(Xw=Xw.astype(np.float32), P2D=uv.astype(np.float32), max_err=(sigma2 * np.float32(5.991)).astype(np.float32), K=K,
                min_inliers=n_min, max_its=its, loop_or=loop_or, quads=quads)
    return prob, R, t


def refine_fail_problem():
    """A problem where Refine fails on a carried-in best mask (outlier matches only) at two qualifying hypotheses whose counts do not
    beat the carried best, and a later hypothesis beats it and returns refined.  Returns (problem, first_qualifying, second, returning)."""
    for seed in range(200):
        p, R, t = synth_problem(80, 600 + seed, outliers=0.3, noise=0.5, min_inliers=10, n_hyp=40, loop_or=False, max_its=40)
        Xc = p["Xw"].astype(np.float64) @ R.T + t
        err = np.sum((project(Xc, p["K"]) - p["P2D"]) ** 2, axis=1)
        bad = np.nonzero(err > 100 * p["max_err"])[0]
        c = ref_ransac(dict(p, min_inliers=80), 5)["hyp_inliers"]   # every count, nothing qualifies
        for v in sorted(set(c.tolist())):
            above = np.nonzero(c > v)[0]
            if v < 8 or not len(above):
                continue
            h = int(above[0])
            for m in range(6, v + 1):
                q = np.nonzero((c[:h] >= m) & (c[:h] <= v))[0]
                if len(q) < 2:
                    continue
                mask = np.zeros(80, bool)
                mask[bad[:6]] = True
                prob = dict(p, min_inliers=m, best_inliers=v, best_mask=mask, best_Tcw=np.full(12, 3, np.float32))
                r = ref_ransac(prob, 5)
                if r["ret_how"] == 1 and r["ret_hyp"] == h:
                    return prob, int(q[0]), int(q[1]), h
    raise RuntimeError("no refine-failure case found")
