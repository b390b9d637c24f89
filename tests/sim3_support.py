"""Test support of the Sim3 check: builds the CPU restatement tests/sim3_ref/sim3_ref.cpp with oracle/Makefile's compiler flags and
makes synthetic loop-closure problems with a known Sim3."""
import ctypes as C
import os
import re
import shlex
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sim3_ref", "sim3_ref.cpp")
_REF = None


def _flags():
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return shlex.split(re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1))


def ref():
    global _REF
    if _REF is None:
        out = os.path.join(tempfile.mkdtemp(prefix="sim3ref"), "libsim3ref.so")
        subprocess.check_call(["g++", *_flags(), "-shared", "-o", out, SRC, "-lm"])
        L = C.CDLL(out)
        L.sim3ref_ransac_its.restype = C.c_int
        L.sim3ref_ransac_its.argtypes = [C.c_int, C.c_double, C.c_int, C.c_int]
        L.sim3ref_optimize.restype = C.c_int
        L.sim3ref_optimize.argtypes = [C.c_int] + [C.c_void_p] * 8 + [C.c_int, C.c_double] + [C.c_void_p] * 4
        _REF = L
    return _REF


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def ref_horn(X1, X2, idx, fix_scale):
    out = np.zeros(37, np.float32)
    ref().sim3ref_horn(_p(np.ascontiguousarray(X1, np.float32)), _p(np.ascontiguousarray(X2, np.float32)),
                       _p(np.ascontiguousarray(idx, np.int32)), C.c_int(int(fix_scale)), _p(out))
    return dict(R=out[:9].reshape(3, 3), t=out[9:12], s=out[12], T12=out[13:25], T21=out[25:37])


def ref_ransac(prob, chunk):
    """The oracle's iterate(chunk) sequence on a problem dict of ydorbslam_amd.sim3.ransac."""
    f = lambda k, w: np.ascontiguousarray(np.asarray(prob[k], np.float32).reshape(-1, w))
    X1, X2, P1, P2, m1, m2 = f("X1", 3), f("X2", 3), f("P1", 2), f("P2", 2), f("max_err1", 1), f("max_err2", 1)
    N = len(X1)
    tri = np.ascontiguousarray(np.asarray(prob["triples"], np.int32).reshape(-1, 3))
    K1, K2 = np.asarray(prob["K1"], np.float32), np.asarray(prob["K2"], np.float32)
    state = np.array([prob.get("next_hyp", 0), prob.get("best_inliers", 0)], np.int32)
    best = np.array(prob.get("best_T12", np.zeros(13)), np.float32)
    out = np.zeros(3, np.int32)
    mask = np.zeros(max(N, 1), np.uint8)
    hyp = np.zeros(max(len(tri), 1), np.int32)
    ref().sim3ref_ransac(C.c_int(N), _p(X1), _p(X2), _p(P1), _p(P2), _p(m1), _p(m2), _p(K1), _p(K2), C.c_int(int(prob["fix_scale"])),
                         C.c_int(prob["min_inliers"]), C.c_int(prob["max_its"]), _p(tri), C.c_int(len(tri)), C.c_int(chunk), _p(state),
                         _p(best), _p(out), _p(mask), _p(hyp))
    return dict(ret_hyp=int(out[0]) if out[0] < 0 else int(out[0]), no_more=bool(out[1]), n_calls=int(out[2]), inliers=mask[:N].astype(bool),
                hyp_inliers=hyp[:len(tri)].copy(), next_hyp=int(state[0]), best_inliers=int(state[1]), best_T12=best)


def ref_optimize(prob, th2=10.0):
    g = lambda k, w: np.ascontiguousarray(np.asarray(prob[k], np.float64).reshape(-1, w))
    X1, X2, o1, o2, w1, w2 = g("X1c", 3), g("X2c", 3), g("obs1", 2), g("obs2", 2), g("inv_sigma2_1", 1), g("inv_sigma2_2", 1)
    E = len(X1)
    S = np.array(prob["S12"], np.float64)
    K1, K2 = np.array(prob["K1"], np.float64), np.array(prob["K2"], np.float64)
    out = np.zeros(max(E, 1), np.uint8)
    chi = np.zeros(2)
    tr = np.zeros(1, np.int32)
    n = ref().sim3ref_optimize(E, _p(X1), _p(X2), _p(o1), _p(o2), _p(w1), _p(w2), _p(K1), _p(K2), int(prob.get("fix_scale", True)), th2,
                               _p(S), _p(out), _p(chi), _p(tr))
    return dict(S12=S, outlier=out[:E].astype(bool), n_in=n, chi2=chi, trials=int(tr[0]))


# ------------------------------------------------------------------------------------------------------------ synthetic problems
def rot(rng, max_angle):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = rng.uniform(-max_angle, max_angle)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def true_sim3(rng, fix_scale):
    R = rot(rng, 0.3)
    t = rng.uniform(-0.5, 0.5, 3)
    s = 1.0 if fix_scale else rng.uniform(0.7, 1.4)
    return R, t, s


K_A = (520.0, 515.0, 320.0, 240.0)
K_B = (480.0, 490.0, 310.0, 250.0)


def synth_ransac(N, seed, fix_scale=True, outliers=0.0, noise=0.5, min_inliers=20, max_its=300, n_hyp=None, K1=K_A, K2=K_B):
    """N pairs related by a known Sim3 (X1 = s R X2 + t), a fraction replaced by random points, pixel noise on the images; returns the
    problem dict of ydorbslam_amd.sim3.ransac (triples drawn by the reference's procedure) and the true (R, t, s)."""
    from ydorbslam_amd.sim3 import RandGen, camera_to_image, draw_triples
    rng = np.random.default_rng(seed)
    R, t, s = true_sim3(rng, fix_scale)
    X1 = np.stack([rng.uniform(-2, 2, N), rng.uniform(-1.5, 1.5, N), rng.uniform(3, 9, N)], axis=1)
    X2 = ((X1 - t) @ R) / s   # R^T (X1 - t) / s
    nb = int(round(outliers * N))
    bad = rng.choice(N, nb, replace=False) if nb else np.zeros(0, int)
    X2[bad] = np.stack([rng.uniform(-2, 2, nb), rng.uniform(-1.5, 1.5, nb), rng.uniform(3, 9, nb)], axis=1)
    X1f, X2f = X1.astype(np.float32), X2.astype(np.float32)
    P1 = camera_to_image(X1f, K1) + rng.normal(0, noise, (N, 2)).astype(np.float32)
    P2 = camera_to_image(X2f, K2) + rng.normal(0, noise, (N, 2)).astype(np.float32)
    oct1, oct2 = rng.integers(0, 8, N), rng.integers(0, 8, N)
    sig = lambda o: (np.float32(1.2) ** (2 * o)).astype(np.float32)
    me1 = np.floor(9.210 * sig(oct1).astype(np.float64)).astype(np.float32)
    me2 = np.floor(9.210 * sig(oct2).astype(np.float64)).astype(np.float32)
    H = max_its if n_hyp is None else n_hyp
    tri = draw_triples(N, H, RandGen(seed)) if N >= 3 else np.zeros((0, 3), np.int32)
    prob = dict(X1=X1f, X2=X2f, P1=P1.astype(np.float32), P2=P2.astype(np.float32), max_err1=me1, max_err2=me2, K1=K1, K2=K2,
                fix_scale=fix_scale, min_inliers=min_inliers, max_its=max_its, triples=tri)
    return prob, (R, t, s)


def quat_xyzw(R):
    w = np.sqrt(max(0.0, 1 + np.trace(R))) / 2
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


def synth_optimize(E, seed, fix_scale=True, outliers=0.0, noise=1.0, init_err=0.02, K1=K_A, K2=K_B):
    """E pairs with a known Sim3 S12 (X1c = s R X2c + t), pixel noise, a fraction of gross outliers, and a perturbed initial S12."""
    rng = np.random.default_rng(seed)
    R, t, s = true_sim3(rng, fix_scale)
    X1 = np.stack([rng.uniform(-2, 2, E), rng.uniform(-1.5, 1.5, E), rng.uniform(3, 9, E)], axis=1)
    X2 = ((X1 - t) @ R) / s
    proj = lambda X, K: np.stack([X[:, 0] / X[:, 2] * K[0] + K[2], X[:, 1] / X[:, 2] * K[1] + K[3]], axis=1)
    o1 = proj(X1, K1) + rng.normal(0, noise, (E, 2))
    o2 = proj(X2, K2) + rng.normal(0, noise, (E, 2))
    nb = int(round(outliers * E))
    if nb:
        bad = rng.choice(E, nb, replace=False)
        o1[bad] += rng.uniform(20, 60, (nb, 2)) * rng.choice([-1, 1], (nb, 2))
    oct1, oct2 = rng.integers(0, 8, E), rng.integers(0, 8, E)
    R0 = rot(rng, init_err) @ R
    S12 = np.concatenate([quat_xyzw(R0), t + rng.normal(0, init_err, 3), [s if fix_scale else s * (1 + rng.normal(0, init_err))]])
    return dict(X1c=X1, X2c=X2, obs1=o1, obs2=o2, inv_sigma2_1=1.2 ** (-2.0 * oct1), inv_sigma2_2=1.2 ** (-2.0 * oct2), K1=K1, K2=K2,
                S12=S12, fix_scale=fix_scale, truth=(R, t, s))
