"""The C++ adapter bodies of the RGB-D constructor's tail (include/ydorb/frame.hpp) EXECUTED on the GPU (tests/cpp_host/frame_run.cpp on a
stand-in Frame that carries data): finishRGBDFrameImpl, and extractAndCompute followed by the four separate bodies, each leave the
frame in the state the CPU restatement predicts from the extractor's keypoints: both keypoint vectors, descriptors, m_v_rightXcords,
m_v_depth, the image bounds and the per-cell vectors; the adapter's sample-gather path equals its image path."""
import os
import subprocess

import numpy as np
import pytest

import frame_support as fs
from frame_support import ROOT, f32

pytestmark = pytest.mark.gpu
SRC = os.path.join(ROOT, "tests", "cpp_host", "frame_run.cpp")
W, H, NF = 320, 240, 500
K, DIST = (229.3, 228.6, 160.4, 119.7), fs.CAMERAS["barrel"][1]
FACTOR = float(f32(1.0) / f32(5000.0))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("frm") / "frame_run")
    lib_dir = os.path.join(ROOT, "ydorbslam_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpu_harness", "mockrt"),
                           "-I" + os.path.join(ROOT, "include"), SRC, "-o", out, "-L" + lib_dir, "-l:libydorb.so", "-Wl,-rpath," + lib_dir])
    return out


def _record(raw, off):
    import ydorbslam_amd as y
    n, st = (int(v) for v in np.frombuffer(raw, np.int32, 2, off))
    off += 8
    r = dict(n=n, status=st)
    for key, dt, count in (("kps_raw", y.KP_DTYPE, n), ("kps_un", y.KP_DTYPE, n), ("desc", np.uint8, 32 * n), ("right_x", f32, n), ("depth", f32, n),
                           ("bounds", f32, 4), ("cell_start", np.int32, 64 * 48 + 1)):
        r[key] = np.frombuffer(raw, dt, count, off)
        off += r[key].nbytes
    r["cell_idx"] = np.frombuffer(raw, np.int32, int(r["cell_start"][-1]), off)
    return r, off + r["cell_idx"].nbytes


@pytest.mark.parametrize("kind", ["u16", "f32", "none"])
def test_adapter_leaves_the_frame_the_restatement_predicts(exe, tmp_path, kind):
    import ydorbslam_amd as y
    from ydorbslam_amd.frame import camera
    from ydorbslam_amd.synth import synth_frame
    gray = synth_frame(W, H, 44)
    u16, flt = (a[0] for a in fs.depth_images((W, H), seed=8))
    depth = {"u16": u16, "f32": flt, "none": None}[kind]
    factor = FACTOR if kind == "u16" else 1.0
    head = np.array([W, H, {"none": 0, "u16": 1, "f32": 2}[kind], NF], np.int32).tobytes() + np.array([*K, *DIST, fs.BF, factor], f32).tobytes()
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(inp, "wb").write(head + gray.tobytes() + (b"" if depth is None else depth.tobytes()))
    subprocess.check_call([exe, inp, outp])
    raw = open(outp, "rb").read()
    a, off = _record(raw, 0)
    b, off = _record(raw, off)
    n = a["n"]
    rx_img, dz_img = np.frombuffer(raw, f32, n, off), np.frombuffer(raw, f32, n, off + 4 * n)
    assert len(raw) == off + 8 * n
    # what the restatement predicts from the extractor's own keypoints
    ex = y.OrbExtractor(NF)
    kps, desc = ex.extract(gray)
    ex.close()
    c = camera(K, DIST)
    bounds = fs.ref_bounds(c, W, H)
    want = fs.ref_tail(c, kps.reshape(1, -1), [len(kps)], depth=None if depth is None else depth[None], factor=factor, bf=fs.BF, bounds=bounds)
    assert n == len(kps) > 100
    for r in (a, b):
        assert r["n"] == n and r["status"] == want["status"][0]
        fs.same_keypoints(r["kps_raw"], kps)
        fs.same_keypoints(r["kps_un"], want["kps_un"][0])
        assert np.array_equal(r["desc"].reshape(n, 32), desc)
        assert np.array_equal(fs.bits(r["right_x"]), fs.bits(want["right_x"][0])) and np.array_equal(fs.bits(r["depth"]), fs.bits(want["depth"][0]))
        assert np.array_equal(fs.bits(r["bounds"]), fs.bits(bounds))
        assert np.array_equal(r["cell_start"], want["cell_start"][0])
        assert np.array_equal(r["cell_idx"], want["cell_idx"][0, :want["cell_start"][0, -1]])
    # the image path of computeStereoFromRGBDImpl equals its sample-gather path
    assert np.array_equal(fs.bits(rx_img), fs.bits(b["right_x"])) and np.array_equal(fs.bits(dz_img), fs.bits(b["depth"]))
    if kind == "none":
        assert (a["depth"] == -1).all() and (a["right_x"] == -1).all()
    else:
        assert (a["depth"] > 0).sum() > 50 and np.abs(a["kps_un"]["x"] - a["kps_raw"]["x"]).max() > 1.0
