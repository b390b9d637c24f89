"""globalBundleAdjustImpl (include/ydorb/optimizer.hpp) EXECUTED on a stand-in map with more keyframes than the dense reduced camera
solve takes (tests/cpp_host/gba_skyline_run.cpp): asked for the dense solver it throws as before, with its default it writes every pose
and point (the GBA fields when loopKeyFrameID != 0), and what it writes is the ctypes path's result on the same graph."""
import os
import subprocess

import numpy as np
import pytest

import ba_skyline_support as K
from ba_skyline_support import ROOT

pytestmark = pytest.mark.gpu
SRC = os.path.join(ROOT, "tests", "cpp_host", "gba_skyline_run.cpp")
N_KF = 3202        # 3 201 free keyframes: one more than the dense solve takes
ITERATIONS = 4
F32 = np.float32


def _build(tmp):
    exe = os.path.join(tmp, "gba_skyline_run")
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
    """The map as the reference holds it: float poses, float points, float keypoints.  Every keyframe starts with the identity rotation
    (its translation off), so that Converter's float 4x4 -> quaternion step is exact and both paths start from the same bits."""
    p = K.trajectory_problem(N_KF, per_kf=2, loop=True, seed=21, noise_px=1.0)
    prob = dict(p)
    prob["poses"] = p["poses"].copy()
    prob["poses"][:, :3] = p["poses"][:, :3].astype(F32).astype(np.float64)
    prob["poses"][:, 3:] = (0.0, 0.0, 0.0, 1.0)
    prob["points"] = p["points"].astype(F32).astype(np.float64)
    prob["meas"] = p["meas"].astype(F32).astype(np.float64)
    prob["camera"] = p["camera"].astype(F32).astype(np.float64)
    i32 = lambda *v: np.array(v, np.int32).tobytes()
    b = [prob["camera"].astype(F32).tobytes(), i32(ITERATIONS, 1), i32(N_KF)]
    for k in range(N_KF):
        T = np.eye(4, dtype=F32)
        T[:3, 3] = prob["poses"][k, :3]
        b += [i32(k), T.tobytes()]
    order = np.argsort(prob["edge_point"], kind="stable")
    ep, eq, meas = prob["edge_pose"][order], prob["edge_point"][order], prob["meas"][order]
    start = np.searchsorted(eq, np.arange(len(prob["points"]) + 1))
    b.append(i32(len(prob["points"])))
    for q in range(len(prob["points"])):
        b += [prob["points"][q].astype(F32).tobytes(), i32(start[q + 1] - start[q])]
        for e in range(start[q], start[q + 1]):
            b += [i32(ep[e]), meas[e].astype(F32).tobytes()]
    return prob, b"".join(b)


def test_adapter_solves_a_map_above_the_dense_limit(tmp_path):
    import ydorbslam_amd as y
    exe = _build(str(tmp_path))
    prob, blob = _scenario()
    scen = str(tmp_path / "scenario.bin")
    open(scen, "wb").write(blob)
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(__import__("torch").__file__), "lib") + ":" + env.get("LD_LIBRARY_PATH", "")
    # asked for the dense solver, the adapter throws as it always did above the limit
    r = subprocess.run([exe, scen, str(tmp_path / "dense.bin"), "dense", "0"], stderr=subprocess.PIPE, text=True, timeout=120, env=env)
    assert r.returncode == 1 and "wider than the solve kernel's LDS (max 19200)" in r.stderr, r.stderr
    got = y.Optimizer.local_bundle_adjust(prob, y.Optimizer.global_options(ITERATIONS, True), solver=0)
    assert got["info"]["solver_used"] == 2 and got["info"]["n_free"] == N_KF - 1 and got["trials"] >= ITERATIONS
    assert got["log"][-1, 0] < got["log"][0, 0]
    want_T = np.tile(np.eye(4, dtype=F32), (N_KF, 1, 1))
    for k in range(N_KF):
        want_T[k, :3, :3] = _rotation(got["poses"][k, 3:]).astype(F32)
        want_T[k, :3, 3] = got["poses"][k, :3].astype(F32)
    want_X = got["points"].astype(F32)
    for loop_id in (0, 7):
        out = str(tmp_path / ("out%d.bin" % loop_id))
        r = subprocess.run([exe, scen, out, "default", str(loop_id)], stderr=subprocess.PIPE, text=True, timeout=120, env=env)
        assert r.returncode == 0, r.stderr
        raw = open(out, "rb").read()
        kf = np.frombuffer(raw, np.dtype([("writes", np.int32), ("gba", np.int32), ("pose", F32, (4, 4)), ("gba_pose", F32, (4, 4))]), N_KF)
        mp = np.frombuffer(raw, np.dtype([("sets", np.int32), ("updates", np.int32), ("gba", np.int32), ("pos", F32, 3), ("gba_pos", F32, 3)]),
                           len(want_X), kf.nbytes)
        assert kf.nbytes + mp.nbytes == len(raw)
        if loop_id == 0:
            assert (kf["writes"] == 1).all() and (kf["gba"] == 0).all() and np.array_equal(kf["pose"], want_T)
            assert (mp["sets"] == 1).all() and (mp["updates"] == 1).all() and np.array_equal(mp["pos"], want_X)
        else:
            assert (kf["writes"] == 0).all() and (kf["gba"] == loop_id).all() and np.array_equal(kf["gba_pose"], want_T)
            assert (mp["sets"] == 0).all() and (mp["gba"] == loop_id).all() and np.array_equal(mp["gba_pos"], want_X)
            assert np.array_equal(mp["pos"], prob["points"].astype(F32))
        moved = np.abs(want_T[1:, :3, 3] - prob["poses"][1:, :3].astype(F32)).max(axis=1) > 1e-5
        assert moved.mean() > 0.9 and np.array_equal(want_T[0, :3, 3], prob["poses"][0, :3].astype(F32))   # keyframe 0 is fixed
