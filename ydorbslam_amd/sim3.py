"""Loop-closure Sim3 check: Sim3Solver (RANSAC over Horn's closed form) and optimizeSim3, on the GPU through the C ABI
(include/ydorb/c_api.h, "Sim3 RANSAC").  Restates ORB-SLAM2's Sim3Solver.cc and Optimizer::OptimizeSim3, which YDORBSLAM
renames; DESIGN.md section 6c lists the assumed spellings."""
import ctypes as C

import numpy as np

from ._lib import YdSim3Batch, YdSim3Problem, check, lib

RAND_MAX = 2147483647   # glibc


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _dot3f(A, X):
    """Rows of A (float32) times X (float32) the way the project's float cv::Mat arithmetic is restated: every product exact in double,
    summed in double in ascending k, rounded once to float."""
    A = np.asarray(A, np.float32).astype(np.float64)
    X = np.asarray(X, np.float32).astype(np.float64)
    return ((A[..., 0] * X[..., 0] + A[..., 1] * X[..., 1]) + A[..., 2] * X[..., 2]).astype(np.float32)


def camera_points(Xw, Tcw):
    """X3Dc = Rcw * Xw + tcw in float (the constructor's transform)."""
    Xw = np.asarray(Xw, np.float32).reshape(-1, 3)
    T = np.asarray(Tcw, np.float32)
    return np.stack([_dot3f(T[r, :3][None, :], Xw) + T[r, 3] for r in range(3)], axis=1).astype(np.float32)


def camera_to_image(Xc, K):
    """FromCameraToImage: fx * x / z + cx, fy * y / z + cy in float."""
    Xc = np.asarray(Xc, np.float32)
    fx, fy, cx, cy = (np.float32(v) for v in K)
    invz = np.float32(1) / Xc[:, 2]
    return np.stack([fx * (Xc[:, 0] * invz) + cx, fy * (Xc[:, 1] * invz) + cy], axis=1).astype(np.float32)


def ransac_iterations(N, probability=0.99, min_inliers=6, max_iterations=300):
    """setRansacParameters' adjusted iteration cap."""
    with np.errstate(all="ignore"):
        epsilon = float(np.float32(min_inliers) / np.float32(N))
        v = np.ceil(np.log(1 - probability) / np.log(np.float64(1) - epsilon ** 3))
    if min_inliers == N:
        its = 1
    else:
        its = int(v) if np.isfinite(v) and abs(v) < 2147483647 else -2147483648   # x86's conversion of NaN / overflow to int
    return max(1, min(its, max_iterations))


class RandGen:
    """A seeded stand-in of the process-global rand() with DUtils::Random::RandomInt on top."""

    def __init__(self, seed=0):
        self.rng = np.random.default_rng(seed)

    def rand(self):
        return int(self.rng.integers(0, RAND_MAX, endpoint=True))

    def random_int(self, lo, hi):
        return int((self.rand() / (RAND_MAX + 1.0)) * (hi - lo + 1)) + lo


def draw_triples(n_pairs, count, gen):
    """iterate()'s draw: three RandomInt picks over the available-index copy, each swap-removed."""
    out = np.zeros((count, 3), np.int32)
    for h in range(count):
        avail = list(range(n_pairs))
        for i in range(3):
            r = gen.random_int(0, len(avail) - 1)
            out[h, i] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


def _problem_struct(d, triples, hyp_out):
    P = YdSim3Problem()
    P.n, P.fix_scale, P.min_inliers, P.max_its = d["n"], int(d["fix_scale"]), d["min_inliers"], d["max_its"]
    P.X1, P.X2, P.P1, P.P2 = _p(d["X1"]), _p(d["X2"]), _p(d["P1"]), _p(d["P2"])
    P.max_err1, P.max_err2 = _p(d["max_err1"]), _p(d["max_err2"])
    P.K1[:] = [float(v) for v in d["K1"]]
    P.K2[:] = [float(v) for v in d["K2"]]
    P.n_hyp = len(triples)
    P.triples = _p(triples)
    P.next_hyp, P.best_inliers = d["next_hyp"], d["best_inliers"]
    P.best_T12[:] = [float(v) for v in d["best_T12"]]
    P.inliers = _p(d["_mask"])
    P.hyp_inliers = _p(hyp_out)
    return P


def _flat(d):
    d = dict(d)
    for k, w in (("X1", 3), ("X2", 3), ("P1", 2), ("P2", 2), ("max_err1", 1), ("max_err2", 1)):
        d[k] = np.ascontiguousarray(np.asarray(d[k], np.float32).reshape(-1, w) if w > 1 else np.asarray(d[k], np.float32).reshape(-1))
    d["n"] = len(d["X1"])
    d.setdefault("next_hyp", 0)
    d.setdefault("best_inliers", 0)
    d.setdefault("best_T12", np.zeros(13, np.float32))
    d["_mask"] = np.zeros(max(d["n"], 1), np.uint8)
    return d


def ransac(problems, chunk=5, device=0):
    """One ydorb_sim3_ransac call over a batch.  Each problem: dict with X1, X2 [N,3], P1, P2 [N,2], max_err1, max_err2 [N], K1, K2 (fx fy
    cx cy), fix_scale, min_inliers, max_its, triples [H,3], and optionally the resumable state next_hyp, best_inliers, best_T12.
    Returns per problem dict(ret_hyp, no_more, n_calls, inliers [N] bool, hyp_inliers [H], next_hyp, best_inliers, best_T12 [13])."""
    ds = [_flat(p) for p in problems]
    tris = [np.ascontiguousarray(np.asarray(p["triples"], np.int32).reshape(-1, 3)) for p in problems]
    hyps = [np.zeros(max(len(t), 1), np.int32) for t in tris]
    arr = (YdSim3Problem * max(len(ds), 1))()
    for i, d in enumerate(ds):
        arr[i] = _problem_struct(d, tris[i], hyps[i])
    check(lib().ydorb_sim3_ransac(arr, len(ds), int(chunk), int(device)))
    out = []
    for i, d in enumerate(ds):
        P = arr[i]
        out.append(dict(ret_hyp=P.ret_hyp, no_more=bool(P.no_more), n_calls=P.n_calls, inliers=d["_mask"][:d["n"]].astype(bool),
                        hyp_inliers=hyps[i][:len(tris[i])].copy(), next_hyp=P.next_hyp, best_inliers=P.best_inliers,
                        best_T12=np.array(P.best_T12[:], np.float32)))
    return out


class Sim3Solver:
    """Sim3Solver(KF1, KF2, matched12, fixScale) on flat data.  Xw1 / Xw2 [M,3]: the world points of KF1's matches and of their partners
    in KF2; valid [M]: the constructor's predicates (both map points set and not bad, both indexed in their keyframe); Tcw1 / Tcw2 3x4;
    kp1 / kp2 [M,2] are not needed (the reference images X3Dc through K); sigma2_1 / sigma2_2 [M]: sigma^2 of each keypoint's octave."""

    def __init__(self, Xw1, Xw2, Tcw1, Tcw2, K1, K2, sigma2_1, sigma2_2, fix_scale=True, valid=None, seed=0):
        M = len(Xw1)
        keep = np.ones(M, bool) if valid is None else np.asarray(valid, bool)
        self.indices1 = np.nonzero(keep)[0].astype(np.int32)
        self.n_matches1 = M
        self.X1 = camera_points(np.asarray(Xw1)[keep], Tcw1)
        self.X2 = camera_points(np.asarray(Xw2)[keep], Tcw2)
        # mvnMaxError is a std::vector<size_t> in the reference: 9.210 * sigma^2 truncated to an integer
        self.max_err1 = np.floor(9.210 * np.asarray(sigma2_1, np.float32)[keep].astype(np.float64)).astype(np.float32)
        self.max_err2 = np.floor(9.210 * np.asarray(sigma2_2, np.float32)[keep].astype(np.float64)).astype(np.float32)
        self.K1, self.K2 = np.asarray(K1, np.float32), np.asarray(K2, np.float32)
        self.P1 = camera_to_image(self.X1, self.K1)
        self.P2 = camera_to_image(self.X2, self.K2)
        self.fix_scale = bool(fix_scale)
        self.gen = RandGen(seed)
        self.set_ransac_parameters()

    @property
    def N(self):
        return len(self.indices1)

    def set_ransac_parameters(self, probability=0.99, min_inliers=6, max_iterations=300):
        self.min_inliers = int(min_inliers)
        self.max_its = ransac_iterations(self.N, probability, min_inliers, max_iterations)
        self.iterations = 0
        self.best_inliers = 0
        self.best_T12 = np.zeros(13, np.float32)

    def problem(self, triples):
        return dict(X1=self.X1, X2=self.X2, P1=self.P1, P2=self.P2, max_err1=self.max_err1, max_err2=self.max_err2, K1=self.K1, K2=self.K2,
                    fix_scale=self.fix_scale, min_inliers=self.min_inliers, max_its=self.max_its, triples=triples,
                    next_hyp=self.iterations, best_inliers=self.best_inliers, best_T12=self.best_T12)

    def draw(self, n):
        """The triples one iterate(n) call draws (none when it would return at once)."""
        if self.N < self.min_inliers:
            return np.zeros((0, 3), np.int32)
        return draw_triples(self.N, max(0, min(n, self.max_its - self.iterations)), self.gen)

    def commit(self, r):
        self.iterations, self.best_inliers, self.best_T12 = r["next_hyp"], r["best_inliers"], r["best_T12"]
        inl = np.zeros(self.n_matches1, bool)
        inl[self.indices1[r["inliers"]]] = True
        T = None
        if r["ret_hyp"] >= 0:
            T = dict(R=r["best_T12"][:9].reshape(3, 3).copy(), t=r["best_T12"][9:12].copy(), s=float(r["best_T12"][12]))
        return T, r["no_more"], inl, int(r["inliers"].sum())

    def iterate(self, n, device=0):
        """iterate(nIterations, bNoMore, vbInliers, nInliers) -> (T12 dict(R, t, s) or None, bNoMore, inliers over KF1's matches, nInliers)."""
        r = ransac([self.problem(self.draw(n))], chunk=max(1, n), device=device)[0]
        return self.commit(r)


def optimize_sim3(problems, th2=10.0, device=0):
    """Optimizer::optimizeSim3 for a batch in one launch.  Each problem: dict with X1c, X2c [E,3] (camera frames of KF1 / KF2), obs1, obs2
    [E,2], inv_sigma2_1, inv_sigma2_2 [E], K1, K2 (fx fy cx cy), S12 [8] = qx qy qz qw tx ty tz s, fix_scale.
    Returns per problem dict(S12 [8], outlier [E] bool, n_in, chi2 [2], trials)."""
    n = len(problems)
    if n == 0:
        return []
    counts = [len(np.asarray(p["inv_sigma2_1"]).reshape(-1)) for p in problems]
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    E = int(start[-1])
    cat = lambda k, w: np.ascontiguousarray(np.concatenate([np.asarray(p[k], np.float64).reshape(-1, w) for p in problems]).reshape(-1, w))
    X1, X2, o1, o2, w1, w2 = cat("X1c", 3), cat("X2c", 3), cat("obs1", 2), cat("obs2", 2), cat("inv_sigma2_1", 1), cat("inv_sigma2_2", 1)
    S = np.ascontiguousarray(np.stack([np.asarray(p["S12"], np.float64) for p in problems]))
    K1 = np.ascontiguousarray(np.stack([np.asarray(p["K1"], np.float64) for p in problems]))
    K2 = np.ascontiguousarray(np.stack([np.asarray(p["K2"], np.float64) for p in problems]))
    fix = np.array([1 if p.get("fix_scale", True) else 0 for p in problems], np.uint8)
    B = YdSim3Batch(n, device, _p(start), _p(S), _p(K1), _p(K2), _p(fix), _p(X1), _p(X2), _p(o1), _p(o2), _p(w1), _p(w2), float(th2))
    outlier = np.zeros(max(E, 1), np.uint8)
    nin = np.zeros(n, np.int32); chi = np.zeros((n, 2), np.float64); trials = np.zeros(n, np.int32)
    check(lib().ydorb_sim3_optimize(C.byref(B), _p(outlier), _p(nin), _p(chi), _p(trials)))
    return [dict(S12=S[i].copy(), outlier=outlier[start[i]:start[i + 1]].astype(bool), n_in=int(nin[i]), chi2=chi[i].copy(),
                 trials=int(trials[i])) for i in range(n)]


def release(device=0):
    """ydorb_sim3_release: give the Sim3 scratch of `device` back."""
    check(lib().ydorb_sim3_release(device))
