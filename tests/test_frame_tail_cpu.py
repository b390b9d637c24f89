"""The CPU restatement of the Frame constructor's tail (tests/frame_ref/frame_ref.cpp) against an independent numpy float64 statement of
the arithmetic contract ("Frame tail"), hand-built rows, a forward-distortion sign guard, the matcher oracle's
grid and the image bounds of the three test cameras.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import frame_support as fs
from frame_support import f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(fs.CAMERAS))
def test_restatement_equals_numpy_statement(name):
    xy = fs.points(name)
    got, st = fs.ref_undistort(fs.cam(name), xy)
    want, broke = fs.numpy_undistort(name, xy)
    assert np.array_equal(fs.bits(got), fs.bits(want))
    assert st == 0 and not broke.any()                    # no icdist < 0 on any of the three cameras
    w, h = fs.size(name)
    outside = (got[:, 0] < 0) | (got[:, 0] >= w) | (got[:, 1] < 0) | (got[:, 1] >= h)
    print(name, "points undistorted to outside the image:", int(outside.sum()))
    if name == "tum_fr1":
        assert not outside.any()
    if name == "barrel":
        assert outside.sum() > 100                        # barrel distortion pushes the border outwards by up to ~140 px
    if name == "pinhole":
        assert np.array_equal(fs.bits(got), fs.bits(xy))  # k1 == 0: the copy exit, although p1 != 0


def test_other_iteration_counts():
    xy = fs.points("tum_fr1", 200)
    for it in (1, 2, 8):
        got, _ = fs.ref_undistort(fs.cam("tum_fr1", it), xy)
        assert np.array_equal(fs.bits(got), fs.bits(fs.numpy_undistort("tum_fr1", xy, it)[0]))


def test_principal_point_stays():
    c = fs.cam("tum_fr1")
    got, st = fs.ref_undistort(c, [[c.cx, c.cy]])
    assert st == 0 and got[0, 0] == f32(c.cx) and got[0, 1] == f32(c.cy)   # x0 = y0 = 0: every iteration leaves 0


def test_negative_icdist_restores_start_and_sets_bit2():
    from ydorbslam_amd.frame import STATUS_ICDIST, camera
    c = camera(fs.TUM_K, (-10.0, 0.0, 0.0, 0.0, 0.0))     # 1 + k1 r2 < 0 from r2 = 0.1 on: 300 px off the centre is r2 = 0.34
    xy = np.array([[18.0, 255.0], [320.0, 256.0]], f32)   # the second point is 1.4 px off the centre: r2 ~ 7e-6, no exit
    got, st = fs.ref_undistort(c, xy)
    assert st == STATUS_ICDIST
    fx, cx = np.float64(f32(fs.TUM_K[0])), np.float64(f32(fs.TUM_K[2]))
    x0 = (np.float64(xy[0, 0]) - cx) * (np.float64(1.0) / fx)
    assert got[0, 0] == f32(fx * x0 + cx)                 # (float)(fx x0 + cx): the start value, not an iterate
    assert abs(float(got[0, 0]) - 18.0) < 1e-3
    o = fs.ref_tail(c, fs.keypoints(xy).reshape(1, 2), [2])
    assert o["status"][0] == STATUS_ICDIST
    assert np.array_equal(fs.bits(o["kps_un"]["x"][0]), fs.bits(got[:, 0]))


def test_depth_rows():
    from ydorbslam_amd.frame import DEPTH_AT_UNDISTORTED, STATUS_DEPTH_INDEX
    c = fs.cam("pinhole")                                 # copy exit: un == raw, so right_x is easy to state
    w, h = 640, 480
    xy = np.array([[10.2, 20.7], [11.0, 20.0], [12.9, 20.0], [13.0, 20.99], [639.99, 479.99], [14.5, 20.5], [640.0, 5.0], [5.0, -1.0],
                   [-0.5, -0.5]], f32)
    kps = fs.keypoints(xy).reshape(1, -1)
    flt = np.full((1, h, w), 2.0, f32)
    flt[0, 20, 10], flt[0, 20, 11], flt[0, 20, 12], flt[0, 20, 13] = 3.0, 0.0, -2.0, np.nan
    flt[0, 479, 639], flt[0, 0, 0] = 5.0, 7.0
    o = fs.ref_tail(c, kps, [len(xy)], flt, bf=fs.BF)
    d, rx = o["depth"][0], o["right_x"][0]
    assert d[0] == 3.0 and rx[0] == f32(xy[0, 0]) - f32(fs.BF) / f32(3.0)   # (int) truncates 10.2, 20.7 to (20, 10)
    assert d[1] == -1 and rx[1] == -1                     # depth 0
    assert d[2] == -1 and rx[2] == -1                     # negative depth
    assert d[3] == -1 and rx[3] == -1                     # NaN fails d > 0
    assert d[4] == 5.0                                    # x = 639.99 is pixel 639
    assert d[5] == 2.0
    assert d[6] == -1 and d[7] == -1                      # x == w and y == -1: outside
    assert d[8] == 7.0                                    # (int)(-0.5) == 0
    assert o["status"][0] == STATUS_DEPTH_INDEX
    assert fs.ref_tail(c, kps[:, :6], [6], flt, bf=fs.BF)["status"][0] == 0
    u16 = np.zeros((1, h, w), np.uint16)
    u16[0, 20, 10], u16[0, 20, 11] = 65535, 5000
    o = fs.ref_tail(c, kps[:, :2], [2], u16, factor=f32(1.0) / f32(5000.0), bf=fs.BF)
    assert o["depth"][0, 0] == f32(65535) * (f32(1.0) / f32(5000.0)) and o["depth"][0, 1] == f32(5000) * (f32(1.0) / f32(5000.0))
    # the sample form is the image form with the look-up done by the caller
    s = np.array([[3.0, 0.0, -2.0, np.nan, 5.0, 2.0, -1.0, -1.0, 7.0]], f32)
    os_ = fs.ref_tail(c, kps, [len(xy)], s, samples=True, bf=fs.BF)
    o = fs.ref_tail(c, kps, [len(xy)], flt, bf=fs.BF)
    assert np.array_equal(fs.bits(os_["depth"]), fs.bits(o["depth"])) and np.array_equal(fs.bits(os_["right_x"]), fs.bits(o["right_x"]))
    # undistorted index: on the barrel camera keypoints leave the image and get no depth
    cb, (bw, bh) = fs.cam("barrel"), fs.size("barrel")
    kb = fs.keypoints(fs.points("barrel", 400)).reshape(1, -1)
    img = np.full((1, bh, bw), 2.5, f32)
    raw, und = fs.ref_tail(cb, kb, [400], img, bf=fs.BF), fs.ref_tail(cb, kb, [400], img, bf=fs.BF, flags=DEPTH_AT_UNDISTORTED)
    assert raw["status"][0] == 0 and (raw["depth"][0] == 2.5).all()
    ux, uy = und["kps_un"]["x"][0], und["kps_un"]["y"][0]
    out = ~((ux > -1) & (ux < bw) & (uy > -1) & (uy < bh))
    assert out.sum() > 20 and und["status"][0] == STATUS_DEPTH_INDEX
    assert (und["depth"][0][out] == -1).all() and (und["right_x"][0][out] == -1).all() and (und["depth"][0][~out] == 2.5).all()


def test_sign_guard_forward_distortion_tum():
    """The only tolerance of the file: forward-distorting the undistorted points must land on the input within 0.05 px (5 iterations
    leave ~0.006 px on TUM fr1; a sign error in any term moves points by pixels)."""
    xy = fs.points("tum_fr1")
    un, _ = fs.ref_undistort(fs.cam("tum_fr1"), xy)
    err = np.abs(fs.distort("tum_fr1", un) - xy).max()
    print("max forward-distortion error, px:", err)
    assert err < 0.05


def _area_from_csr(kps, bounds, cs, ci, x, y, r):
    """Frame::getKeyPointsInArea (frame.cpp:337-361, no level window) over a CSR grid, in float32 like the oracle."""
    minx, maxx, miny, maxy = (f32(b) for b in bounds)
    gw, gh = f32(64) / (maxx - minx), f32(48) / (maxy - miny)
    x, y, r = f32(x), f32(y), f32(r)
    c0, c1 = max(0, int(np.floor((x - minx - r) * gw))), min(63, int(np.ceil((x - minx + r) * gw)))
    r0, r1 = max(0, int(np.floor((y - miny - r) * gh))), min(47, int(np.ceil((y - miny + r) * gh)))
    out = []
    for ix in range(c0, c1 + 1):
        for iy in range(r0, r1 + 1):
            for idx in ci[cs[ix * 48 + iy]:cs[ix * 48 + iy + 1]]:
                if abs(kps["x"][idx] - x) > r and abs(kps["y"][idx] - y) < r:
                    out.append(int(idx))
    return out


def test_grid_equals_matcher_oracle_on_barrel():
    """The oracle keeps its grid to itself, so it is read through getKeyPointsInArea: one query per keypoint, placed so that the keypoint
    passes the area test's filter (x distance above r, y distance below r) and its cell lies in the window, although the cell rule
    offsets y by min_x and the window by min_y.  Every answer must equal the same query over the restatement's CSR, and a keypoint
    must turn up in its own query exactly when the CSR holds it."""
    from oracle.orb_oracle import FrameOracle
    name = "barrel"
    c, (w, h) = fs.cam(name), fs.size(name)
    bounds = fs.ref_bounds(c, w, h)
    kps = fs.keypoints(fs.points(name)).reshape(1, -1)
    n = kps.shape[1]
    o = fs.ref_tail(c, kps, [n], bounds=bounds)
    un, cs, ci = o["kps_un"][0], o["cell_start"][0], o["cell_idx"][0]
    held = np.zeros(n, bool)
    held[ci[:cs[-1]]] = True
    print("keypoints outside the grid:", int((~held).sum()))
    assert 0 < (~held).sum() < 100 and cs[-1] == held.sum()
    for c_ in np.nonzero(np.diff(cs))[0]:
        assert (np.diff(ci[cs[c_]:cs[c_ + 1]]) > 0).all()          # push_back order
    fo = FrameOracle(un, np.zeros((n, 32), np.uint8), bounds)
    r = 100.0
    for i in range(n):
        x, y = float(un["x"][i]) - (r + 0.5), float(un["y"][i])
        got = fo.keypoints_in_area(x, y, r).tolist()
        assert got == _area_from_csr(un, bounds, cs, ci, x, y, r), i
        assert (i in got) == bool(held[i]), i


def test_image_bounds():
    table = {"tum_fr1": ((10.80, 626.05, 14.67, 473.31), 0.006), "barrel": ((-135.8, 895.5, -92.9, 565.6), 0.06)}   # half a unit of the last digit given
    for name in sorted(fs.CAMERAS):
        c, (w, h) = fs.cam(name), fs.size(name)
        b = fs.ref_bounds(c, w, h)
        if name == "pinhole":
            assert b.tolist() == [0.0, float(w), 0.0, float(h)]
            continue
        un, _ = fs.numpy_undistort(name, np.array([[0, 0], [w, 0], [0, h], [w, h]], f32))
        want = np.array([min(un[0, 0], un[2, 0]), max(un[1, 0], un[3, 0]), min(un[0, 1], un[1, 1]), max(un[2, 1], un[3, 1])], f32)
        assert np.array_equal(fs.bits(b), fs.bits(want))
        print(name, b)
        assert np.abs(b - np.array(table[name][0])).max() < table[name][1]


def test_adapter_syntax_check_compiles():
    """include/ydorb/frame.hpp against declaration-only mocks of the reference's Frame and of OpenCV."""
    h = os.path.join(ROOT, "tests", "cpu_harness")
    subprocess.check_call(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-I" + os.path.join(h, "mock"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(h, "frame_syntax_check.cpp")])
