"""The C++ adapter include/ydorb/pnpSolver.hpp EXECUTED on the GPU (tests/cpp_host/pnp_run.cpp on stand-ins of Frame / MapPoint that
carry data): the constructor's predicates, mvKeyPointIndices and maxError, setRansacParameters, the RandomInt draw from rand() with the
||/&& sequence length, the state carried between iterate() calls, and pnpIterateBatch over several candidates; every call equals the
ctypes path (ydorbslam_amd.pnp.ransac) on the same flat problem with the same quads."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from pnp_support import K_VGA, ROOT, synth_scene

pytestmark = pytest.mark.gpu
SRC = os.path.join(ROOT, "tests", "cpp_host", "pnp_run.cpp")
SIG2 = (np.float32(1.2) ** (2 * np.arange(8))).astype(np.float32)
TH2 = np.float32(5.991)


def _build(tmp):
    exe = os.path.join(tmp, "pnp_run")
    lib_dir = os.path.join(ROOT, "ydorbslam_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpu_harness", "mockrt"),
                           "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe, "-L" + lib_dir, "-l:libydorb.so", "-Wl,-rpath," + lib_dir])
    return exe


def _scene(seed, outliers, nKP=160):
    """Keypoint i images map point i (pixel noise by octave); each match vector maps a fraction of keypoints to a wrong point and
    leaves some unmatched; a few map points are bad."""
    rng = np.random.default_rng(seed)
    pos, uv, _, _ = synth_scene(nKP, seed)
    octv = rng.integers(0, 8, nKP).astype(np.int32)
    kps = (uv + rng.normal(0, 0.5, (nKP, 2)) * np.sqrt(SIG2[octv])[:, None]).astype(np.float32)
    bad = rng.uniform(size=nKP) < 0.05
    matches = []
    for o in outliers:
        m = np.arange(nKP, dtype=np.int32)
        out = rng.uniform(size=nKP) < o
        m[out] = rng.integers(0, nKP, out.sum())
        m[rng.uniform(size=nKP) < 0.05] = -1
        matches.append(m)
    return dict(pos=pos.astype(np.float32), kps=kps, octv=octv, bad=bad, matches=matches)


def _blob(s, loop_or, seed):
    nKP = len(s["kps"])
    b = [np.array([nKP, len(s["pos"]), len(s["matches"]), int(loop_or), seed], np.int32).tobytes(),
         np.array(K_VGA, np.float32).tobytes(), SIG2.tobytes()]
    rec = np.zeros(nKP, [("x", "<f4"), ("y", "<f4"), ("o", "<i4")])
    rec["x"], rec["y"], rec["o"] = s["kps"][:, 0], s["kps"][:, 1], s["octv"]
    b.append(rec.tobytes())
    rec = np.zeros(len(s["pos"]), [("p", "<f4", 3), ("bad", "<i4")])
    rec["p"], rec["bad"] = s["pos"], s["bad"]
    b.append(rec.tobytes())
    b += [m.tobytes() for m in s["matches"]]
    return b"".join(b)


def _flat(s, k):
    """The constructor restated: matches with a map point that is not bad, in keypoint order."""
    m = s["matches"][k]
    keep = np.array([i for i in range(len(m)) if m[i] >= 0 and not s["bad"][m[i]]], np.int32)
    sig = SIG2[s["octv"][keep]]
    return dict(indices=keep, Xw=s["pos"][m[keep]], P2D=s["kps"][keep], max_err=(sig * TH2).astype(np.float32))


class _Out:
    def __init__(self, path):
        self.raw, self.at = open(path, "rb").read(), 0

    def get(self, dt, n=1):
        a = np.frombuffer(self.raw, dt, n, self.at)
        self.at += a.nbytes
        return a

    def solver(self):
        N = int(self.get("<i4")[0])
        return dict(N=N, indices=self.get("<i4", N), Xw=self.get("<f4", 3 * N), P2D=self.get("<f4", 2 * N), max_err=self.get("<f4", N),
                    min_inliers=int(self.get("<i4")[0]), max_its=int(self.get("<i4")[0]))

    def call(self, nKP):
        k, nq = int(self.get("<i4")[0]), int(self.get("<i4")[0])
        quads = self.get("<i4", 4 * nq).reshape(-1, 4)
        ret, no_more, n_inl, n_vb = (int(v) for v in self.get("<i4", 4))
        return dict(k=k, quads=quads, ret=ret, no_more=no_more, n_inl=n_inl, n_vb=n_vb, inl=self.get("u1", nKP).astype(bool),
                    T=self.get("<f4", 16))

    def done(self):
        return self.at == len(self.raw)


class _Replay:
    """One candidate on the ctypes path: draws from the glibc stream as the adapter does, carries the state between calls."""

    def __init__(self, f, nKP, loop_or):
        from ydorbslam_amd.pnp import ransac_parameters
        self.f, self.nKP, self.loop_or = f, nKP, loop_or
        self.N = len(f["indices"])
        self.min_inl, self.max_its, _ = ransac_parameters(self.N, 0.99, 10, 300, 4, 0.5)
        self.state = dict(next_hyp=0, best_inliers=0, best_mask=np.zeros(self.N, bool), best_Tcw=np.zeros(12, np.float32))

    def draw(self, rand_int):
        from ydorbslam_amd.pnp import call_length
        q = []
        if self.N >= 4:
            for _ in range(call_length(self.N, self.min_inl, self.max_its, self.state["next_hyp"], 5, self.loop_or)):
                avail = list(range(self.N))
                for _ in range(4):
                    r = rand_int(0, len(avail) - 1)
                    q.append(avail[r]); avail[r] = avail[-1]; avail.pop()
        return np.array(q, np.int32).reshape(-1, 4)

    def problem(self, quads):
        return dict(Xw=self.f["Xw"], P2D=self.f["P2D"], max_err=self.f["max_err"], K=K_VGA, min_inliers=self.min_inl,
                    max_its=self.max_its, loop_or=self.loop_or, quads=quads, **self.state)

    def check(self, r, quads, g):
        """r: the ctypes result of this call; g: the adapter's record of it.  Returns True when iterate returned or set bNoMore."""
        self.state = dict(next_hyp=r["next_hyp"], best_inliers=r["best_inliers"], best_mask=r["best_mask"], best_Tcw=r["best_Tcw"])
        assert np.array_equal(g["quads"], quads)
        assert g["ret"] == (r["ret_how"] != 0) and g["no_more"] == r["no_more"]
        if g["ret"]:
            inl = np.zeros(self.nKP, bool)
            inl[self.f["indices"][r["inliers"]]] = True
            assert np.array_equal(g["inl"], inl) and g["n_inl"] == r["n_inliers"] and g["n_vb"] == self.nKP
            T = np.zeros(16, np.float32)
            T[:12] = r["Tcw"]
            T[15] = 1
            assert np.array_equal(g["T"].view(np.uint32), T.view(np.uint32))
        else:
            assert not g["inl"].any() and g["n_inl"] == 0 and g["n_vb"] == 0
        return g["ret"] == 1 or g["no_more"] == 1


def _rand_stream(seed, n):
    libc = C.CDLL(None)
    libc.rand.restype = C.c_int
    libc.srand(C.c_uint(seed))
    stream = iter([libc.rand() for _ in range(n)])
    return lambda lo, hi: int((next(stream) / (2147483647 + 1.0)) * (hi - lo + 1)) + lo


def _check_solver(g, f):
    from ydorbslam_amd.pnp import ransac_parameters
    assert np.array_equal(g["indices"], f["indices"])
    for k in ("Xw", "P2D", "max_err"):
        assert np.array_equal(g[k].view(np.uint32), np.ascontiguousarray(f[k]).reshape(-1).view(np.uint32)), k
    assert (g["min_inliers"], g["max_its"]) == ransac_parameters(g["N"], 0.99, 10, 300, 4, 0.5)[:2]


@pytest.mark.parametrize("loop_or,outliers", [(False, 0.6), (False, 0.3), (True, 0.3), (True, 0.6)])
def test_iterate_sequence_equals_ctypes(tmp_path, loop_or, outliers):
    from ydorbslam_amd.pnp import ransac
    exe = _build(str(tmp_path))
    s = _scene(41 + int(10 * outliers), [outliers])
    seed = 777
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(inp, "wb").write(_blob(s, loop_or, seed))
    subprocess.check_call([exe, "seq", inp, outp])
    nKP = len(s["kps"])
    out = _Out(outp)
    g0 = out.solver()
    f = _flat(s, 0)
    _check_solver(g0, f)
    rand_int = _rand_stream(seed, 4 * 400 * 300)
    rp = _Replay(f, nKP, loop_or)
    calls = 0
    while True:
        g = out.call(nKP)
        q = rp.draw(rand_int)
        r = ransac([rp.problem(q)], chunk=5)[0]
        calls += 1
        if rp.check(r, q, g):
            break
    assert out.done()
    if not loop_or and outliers == 0.6:   # minInliers = N/2 is out of reach: iterate(5) resumed until bNoMore, maxIts / 5 calls
        assert calls == (rp.max_its + 4) // 5 > 1 and g["no_more"] and not g["ret"]
    if outliers == 0.3:                   # the true pose is found
        assert g["ret"] == 1


@pytest.mark.parametrize("loop_or", [True, False])
def test_iterate_batch_equals_ctypes(tmp_path, loop_or):
    from ydorbslam_amd.pnp import ransac
    exe = _build(str(tmp_path))
    fracs = [0.2, 0.6, 0.4, 0.7, 0.3, 0.55]
    s = _scene(90 + int(loop_or), fracs)
    seed = 4242
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(inp, "wb").write(_blob(s, loop_or, seed))
    subprocess.check_call([exe, "batch", inp, outp])
    nKP = len(s["kps"])
    out = _Out(outp)
    reps = []
    for k in range(len(fracs)):
        f = _flat(s, k)
        _check_solver(out.solver(), f)
        reps.append(_Replay(f, nKP, loop_or))
    rand_int = _rand_stream(seed, 4 * 400 * 300 * len(fracs))
    live = list(range(len(fracs)))
    rounds, returned = 0, 0
    while live:
        quads = [reps[k].draw(rand_int) for k in live]   # prepare() draws in solver order before the one call
        rs = ransac([reps[k].problem(q) for k, q in zip(live, quads)], chunk=5)
        rounds += 1
        nxt = []
        for k, q, r in zip(live, quads, rs):
            g = out.call(nKP)
            assert g["k"] == k
            if reps[k].check(r, q, g):
                returned += g["ret"]
            else:
                nxt.append(k)
        live = nxt
    assert out.done()
    assert returned >= 3   # the candidates with 20 / 30 / 40 % outliers find the pose
    if not loop_or:
        assert rounds > 1  # && resumes the candidates that neither return nor run out in the first round
