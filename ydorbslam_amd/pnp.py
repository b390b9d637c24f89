"""Relocalisation EPnP RANSAC: PnPsolver (RANSAC over Lepetit's EPnP with Refine) on the GPU through the C ABI
(include/ydorb/c_api.h, "EPnP RANSAC").  Restates ORB-SLAM2's PnPsolver.cc, which YDORBSLAM renames to pnpSolver.*; DESIGN.md
section 6d lists the assumed spellings."""
import ctypes as C

import numpy as np

from ._lib import YdPnpProblem, check, lib
from .sim3 import RandGen  # noqa: F401  (the same rand() / RandomInt stand-in)

RET_NONE, RET_REFINED, RET_BEST = 0, 1, 2


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def ransac_parameters(N, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4):
    """SetRansacParameters' arithmetic: (mRansacMinInliers, mRansacMaxIts, mRansacEpsilon as float)."""
    eps = np.float32(epsilon)
    n_min = int(np.float32(N) * eps) if N > 0 else 0   # int nMinInliers = N * mRansacEpsilon (float product, truncated)
    n_min = max(n_min, int(min_inliers), int(min_set))
    with np.errstate(all="ignore"):
        q = np.float32(n_min) / np.float32(N) if N > 0 else np.float32(np.inf)
    if eps < q:
        eps = q
    if n_min == N:
        its = 1
    else:
        with np.errstate(all="ignore"):
            v = np.ceil(np.log(1 - probability) / np.log(1 - np.float64(eps) ** 3))
        its = int(v) if np.isfinite(v) and abs(v) < 2147483647 else -2147483648   # x86's conversion of NaN / overflow to int
    return n_min, max(1, min(its, int(max_iterations))), float(eps)


def ransac_iterations(N, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4):
    """setRansacParameters' adjusted iteration cap mRansacMaxIts."""
    return ransac_parameters(N, probability, min_inliers, max_iterations, min_set, epsilon)[1]


def draw_quads(n_points, count, gen):
    """iterate()'s draw: four RandomInt picks over the available-index copy, each swap-removed."""
    out = np.zeros((count, 4), np.int32)
    for h in range(count):
        avail = list(range(n_points))
        for i in range(4):
            r = gen.random_int(0, len(avail) - 1)
            out[h, i] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


def sequence_length(N, min_inliers, max_its, next_hyp, chunk, loop_or=True):
    """Hypotheses the iterate(chunk) sequence of one ydorb_pnp_ransac call runs without a return (0 when N < minInliers)."""
    if N < min_inliers:
        return 0
    return max(max_its - next_hyp, chunk) if loop_or else max(0, max_its - next_hyp)


def call_length(N, min_inliers, max_its, next_hyp, n, loop_or=True):
    """Hypotheses ONE iterate(n) call runs without a return: with ||, until mnIterations >= maxIts and n have run; with &&, n or what
    maxIts leaves.  0 when N < minInliers."""
    if N < min_inliers:
        return 0
    return max(max_its - next_hyp, n) if loop_or else min(n, max(0, max_its - next_hyp))


def _flat(d):
    d = dict(d)
    d["Xw"] = np.ascontiguousarray(np.asarray(d["Xw"], np.float32).reshape(-1, 3))
    d["P2D"] = np.ascontiguousarray(np.asarray(d["P2D"], np.float32).reshape(-1, 2))
    d["max_err"] = np.ascontiguousarray(np.asarray(d["max_err"], np.float32).reshape(-1))
    d["n"] = n = len(d["Xw"])
    d.setdefault("next_hyp", 0)
    d.setdefault("best_inliers", 0)
    d.setdefault("loop_or", True)
    d["_best_mask"] = np.zeros(max(n, 1), np.uint8)
    if d.get("best_mask") is not None:
        d["_best_mask"][:n] = np.asarray(d["best_mask"], bool)
    d["_best_Tcw"] = np.asarray(d.get("best_Tcw", np.zeros(12)), np.float32).reshape(12)
    d["_mask"] = np.zeros(max(n, 1), np.uint8)
    return d


def _problem_struct(d, quads, hyp_out):
    P = YdPnpProblem()
    P.n, P.min_inliers, P.max_its, P.loop_or = d["n"], int(d["min_inliers"]), int(d["max_its"]), int(bool(d["loop_or"]))
    P.Xw, P.P2D, P.max_err = _p(d["Xw"]), _p(d["P2D"]), _p(d["max_err"])
    P.K[:] = [float(v) for v in d["K"]]
    P.n_hyp = len(quads)
    P.quads = _p(quads)
    P.next_hyp, P.best_inliers = int(d["next_hyp"]), int(d["best_inliers"])
    P.best_mask = _p(d["_best_mask"])
    P.best_Tcw[:] = [float(v) for v in d["_best_Tcw"]]
    P.inliers = _p(d["_mask"])
    P.hyp_inliers = _p(hyp_out)
    return P


def ransac(problems, chunk=5, device=0):
    """One ydorb_pnp_ransac call over a batch.  Each problem: dict with Xw [N,3], P2D [N,2], max_err [N], K (fu fv uc vc), min_inliers,
    max_its, quads [H,4], loop_or (default True: ORB-SLAM2's ||), and optionally the resumable state next_hyp, best_inliers,
    best_mask [N], best_Tcw [12].  Returns per problem dict(ret_hyp, ret_how, no_more, n_calls, Tcw [12], n_inliers, inliers [N] bool,
    hyp_inliers [H], next_hyp, best_inliers, best_mask [N] bool, best_Tcw [12])."""
    ds = [_flat(p) for p in problems]
    quads = [np.ascontiguousarray(np.asarray(p["quads"], np.int32).reshape(-1, 4)) for p in problems]
    hyps = [np.zeros(max(len(q), 1), np.int32) for q in quads]
    arr = (YdPnpProblem * max(len(ds), 1))()
    for i, d in enumerate(ds):
        arr[i] = _problem_struct(d, quads[i], hyps[i])
    check(lib().ydorb_pnp_ransac(arr, len(ds), int(chunk), int(device)))
    out = []
    for i, d in enumerate(ds):
        P, n = arr[i], d["n"]
        out.append(dict(ret_hyp=P.ret_hyp, ret_how=P.ret_how, no_more=bool(P.no_more), n_calls=P.n_calls,
                        Tcw=np.array(P.Tcw[:], np.float32), n_inliers=P.n_inliers, inliers=d["_mask"][:n].astype(bool),
                        hyp_inliers=hyps[i][:len(quads[i])].copy(), next_hyp=P.next_hyp, best_inliers=P.best_inliers,
                        best_mask=d["_best_mask"][:n].astype(bool), best_Tcw=np.array(P.best_Tcw[:], np.float32)))
    return out


class PnPsolver:
    """PnPsolver(F, vpMapPointMatches) on flat data.  Xw [M,3]: world positions of the matched map points; P2D [M,2]: the frame's
    undistorted keypoints; sigma2 [M]: mvLevelSigma2 of each keypoint's octave; valid [M]: the constructor's predicate (map point set
    and not bad); K = (fx, fy, cx, cy).  rand() is a seeded RandGen."""

    def __init__(self, Xw, P2D, sigma2, K, valid=None, seed=0):
        M = len(Xw)
        keep = np.ones(M, bool) if valid is None else np.asarray(valid, bool)
        self.key_point_indices = np.nonzero(keep)[0].astype(np.int32)
        self.n_matches = M
        self.Xw = np.ascontiguousarray(np.asarray(Xw, np.float32).reshape(-1, 3)[keep])
        self.P2D = np.ascontiguousarray(np.asarray(P2D, np.float32).reshape(-1, 2)[keep])
        self.sigma2 = np.asarray(sigma2, np.float32).reshape(-1)[keep]
        self.K = np.asarray(K, np.float32)
        self.gen = RandGen(seed)
        self.set_ransac_parameters()

    @property
    def N(self):
        return len(self.key_point_indices)

    def set_ransac_parameters(self, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4, th2=5.991,
                              loop_or=True):
        self.min_inliers, self.max_its, self.epsilon = ransac_parameters(self.N, probability, min_inliers, max_iterations, min_set,
                                                                         epsilon)
        self.max_err = (self.sigma2 * np.float32(th2)).astype(np.float32)
        self.loop_or = bool(loop_or)
        self.iterations = 0
        self.best_inliers = 0
        self.best_mask = np.zeros(self.N, bool)
        self.best_Tcw = np.zeros(12, np.float32)

    def problem(self, quads):
        return dict(Xw=self.Xw, P2D=self.P2D, max_err=self.max_err, K=self.K, min_inliers=self.min_inliers, max_its=self.max_its,
                    loop_or=self.loop_or, quads=quads, next_hyp=self.iterations, best_inliers=self.best_inliers,
                    best_mask=self.best_mask, best_Tcw=self.best_Tcw)

    def draw(self, n):
        """The quads one iterate(n) call may use, drawn up front (none when it would return at once)."""
        if self.N < 4:   # no set of four can be drawn
            return np.zeros((0, 4), np.int32)
        H = call_length(self.N, self.min_inliers, self.max_its, self.iterations, max(1, n), self.loop_or)
        return draw_quads(self.N, H, self.gen)

    def commit(self, r):
        self.iterations, self.best_inliers = r["next_hyp"], r["best_inliers"]
        self.best_mask, self.best_Tcw = r["best_mask"], r["best_Tcw"]
        inl = np.zeros(self.n_matches, bool)
        inl[self.key_point_indices[r["inliers"]]] = True
        T = None
        if r["ret_how"] != RET_NONE:
            T = np.eye(4, dtype=np.float32)
            T[:3, :] = r["Tcw"].reshape(3, 4)
        no_more = r["no_more"] or (self.min_inliers <= self.N < 4)   # as the adapter: no set can be drawn
        return T, no_more, inl, int(r["n_inliers"])

    def iterate(self, n, device=0):
        """iterate(nIterations, bNoMore, vbInliers, nInliers) -> (Tcw 4x4 float or None, bNoMore, inliers over the matches, nInliers)."""
        return iterate_batch([self], n, device)[0]


def iterate_batch(solvers, n, device=0):
    """iterate(n) on every solver in one ydorb_pnp_ransac call (the relocalisation loop's batch over candidate keyframes)."""
    if not solvers:
        return []
    rs = ransac([s.problem(s.draw(n)) for s in solvers], chunk=max(1, n), device=device)
    return [s.commit(r) for s, r in zip(solvers, rs)]


def release(device=0):
    """ydorb_pnp_release: give the EPnP scratch of `device` back."""
    check(lib().ydorb_pnp_release(device))
