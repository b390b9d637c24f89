"""optimizeEssentialGraphImpl (include/ydorb/optimizer.hpp) EXECUTED on a stand-in map with more keyframes than the dense solver takes
(tests/cpp_host/essgraph_skyline_run.cpp): with its default solver the adapter no longer throws there, writes every pose and point back,
and what it writes is the ctypes path's result on the graph it built.  Asked for the dense solver it fails as before."""
import os
import subprocess

import numpy as np
import pytest

import essgraph_support as S
from essgraph_support import ROOT

pytestmark = pytest.mark.gpu
SRC = os.path.join(ROOT, "tests", "cpp_host", "essgraph_skyline_run.cpp")
N_KF = 2760   # 2 759 free keyframes: the smallest round figure above the dense solver's 2 742
N_MP = 300


def _build(tmp):
    exe = os.path.join(tmp, "essgraph_skyline_run")
    lib_dir = os.path.join(ROOT, "ydorbslam_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpu_harness", "mockrt"),
                           "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe, "-L" + lib_dir, "-l:libydorb.so", "-Wl,-rpath," + lib_dir])
    return exe


def _rotation(q):
    """Eigen's Quaternion::toRotationMatrix in its operation order"""
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def _scenario():
    """A chain of keyframes (parent = the one before), covisible with the two before, the last one closing the loop onto the first."""
    n = N_KF
    rng = np.random.default_rng(8)
    g = S.make_graph(n, [(0, 1)], 78, True, drift=0.002)
    i32 = lambda *v: np.array(v, np.int32).tobytes()
    b = [i32(n)]
    for i in range(n):
        b += [i32(i, 0, i - 1), _rotation(g["sim3"][i][:4]).astype(np.float32).tobytes(), g["sim3"][i][4:7].astype(np.float32).tobytes()]
    covis = [(i, i - 1, 200) for i in range(1, n)] + [(i, i - 2, 150) for i in range(2, n)]
    b.append(i32(len(covis)))
    b.append(np.array(covis, np.int32).tobytes())
    b.append(i32(0))   # no earlier loop edges
    as_sim3 = lambda s: np.concatenate([s[:7], [1.0]])
    for pose in (as_sim3(g["truth"][n - 1]), as_sim3(g["sim3"][n - 1])):   # corrected, non-corrected: the current keyframe
        b += [i32(1), i32(n - 1), pose.tobytes()]
    b += [i32(1), i32(n - 1, 1), i32(0)]   # loop connections: current -> loop keyframe
    pos = rng.uniform(-6, 6, (N_MP, 3)).astype(np.float32)
    ref = rng.integers(0, n, N_MP).astype(np.int32)
    ref[0] = 0
    b.append(i32(N_MP))
    for k in range(N_MP):
        b += [pos[k].tobytes(), i32(0, ref[k], -1, -1)]
    b.append(i32(0, n - 1, 1))
    return b"".join(b), pos, ref


def test_adapter_solves_a_map_above_the_dense_limit(tmp_path):
    from ydorbslam_amd.essential_graph import optimize_essential_graph, plan
    exe = _build(str(tmp_path))
    blob, pos, ref = _scenario()
    scen, out = str(tmp_path / "scenario.bin"), str(tmp_path / "out.bin")
    open(scen, "wb").write(blob)
    # asked for the dense solver, the adapter throws as it always did above the limit
    r = subprocess.run([exe, scen, str(tmp_path / "dense.bin"), "dense"], stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 1 and "at most 2742" in r.stderr, r.stderr
    # its default does not
    r = subprocess.run([exe, scen, out, "auto"], stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    raw = open(out, "rb").read()
    off = [0]

    def take(dtype, n):
        a = np.frombuffer(raw, dtype, n, off[0]).copy()
        off[0] += a.nbytes
        return a

    V = int(take(np.int32, 1)[0])
    sim3, fixed = take(np.float64, 8 * V).reshape(V, 8), take(np.uint8, V)
    E = int(take(np.int32, 1)[0])
    v0, v1, meas = take(np.int32, E), take(np.int32, E), take(np.float64, 8 * E).reshape(E, 8)
    assert V == N_KF and fixed.tolist() == [1] + [0] * (N_KF - 1)
    assert E == 1 + (N_KF - 1) + (N_KF - 2)   # the loop connection, the spanning tree, the covisibility chords to i - 2
    edges = np.stack([v0, v1], axis=1)
    info = plan(sim3, fixed, edges, meas)
    assert info["solver_used"] == "skyline" and info["n_free"] == N_KF - 1
    got = optimize_essential_graph(sim3, fixed, edges, meas, pos, ref, fix_scale=True, solver="auto")
    assert got["info"]["solver_used"] == "skyline"
    chi0 = S.ref_chi2(dict(edges=edges, meas=meas), sim3)
    # the drift was spread over the loop: the chain's measurements contradict the loop edge, so chi2 falls by about the loop's length, not to 0
    print("chi2 %.3e -> %.3e, trials %s" % (chi0, got["log_chi2"][-1], got["log_trials"].tolist()))
    assert got["log_chi2"][-1] < 0.01 * chi0
    moved = 0
    for i in range(N_KF):
        written = int(take(np.int32, 1)[0])
        T = take(np.float32, 16).reshape(4, 4)
        s = got["sim3"][i]
        want_T = np.eye(4, dtype=np.float32)
        want_T[:3, :3] = _rotation(s[:4]).astype(np.float32)
        want_T[:3, 3] = (s[4:7] * (1.0 / s[7])).astype(np.float32)
        assert written == 1 and np.array_equal(T, want_T), i
    for k in range(N_MP):
        n_set, n_upd = take(np.int32, 2)
        p = take(np.float32, 3)
        assert n_set == 1 and n_upd == 1 and np.array_equal(p, got["points"][k]), k
        moved += int(np.abs(p - pos[k]).max() > 1e-4)
    assert moved > N_MP // 2 and np.array_equal(got["points"][0], pos[0])   # the fixed keyframe's point comes back as it went
    assert off[0] == len(raw)
