"""The Frame constructor's tail on the GPU (ydorbslam_amd/csrc/frame_tail.hip) against its CPU restatement (tests/frame_ref), bit for bit:
the batch kernels for every camera, depth source and depth-index flag, the bare undistortion, the image bounds, the grid CSR, the
device-pointer form chained behind the extractor and in front of the matcher, the per-frame single call, arena growth, release and
the argument checks."""
import ctypes as C

import numpy as np
import pytest

import frame_support as fs
from frame_support import f32

pytestmark = pytest.mark.gpu

SOURCES = ("u16", "f32", "samples", "none")
FACTOR = float(f32(1.0) / f32(5000.0))


@pytest.fixture(scope="module")
def images():
    """Depth images of both sizes, in arrays whose rows are longer than the images': {(w, h): (uint16 view, float32 view)}."""
    return {shape: tuple(fs.padded(a) for a in fs.depth_images(shape)) for shape in ((752, 480), (64, 48))}


def _run_both(name, source, flags, depth):
    from ydorbslam_amd.frame import frame_tail
    c, (w, h) = fs.cam(name), fs.size(name)
    kps, n = fs.batch(name)
    bounds = fs.ref_bounds(c, w, h)
    kw = dict(depth=depth, samples=source == "samples", factor=FACTOR if source == "u16" else 1.0, bf=fs.BF, bounds=bounds, flags=flags)
    got, want = frame_tail(c, kps, n, **kw), fs.ref_tail(c, kps, n, **kw)
    fs.same_tail(got, want, n)
    return got, want, kps, n


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("name", sorted(fs.CAMERAS))
def test_batch_equals_restatement(name, source, flags, images):
    from ydorbslam_amd.frame import STATUS_DEPTH_INDEX
    if source in ("u16", "f32"):
        for shape in ((752, 480), (64, 48)):
            depth = images[shape][0 if source == "u16" else 1]
            assert depth.strides[1] > depth.shape[2] * depth.itemsize          # a row stride larger than the row
            got, want, kps, n = _run_both(name, source, flags, depth)
            if shape == (64, 48):
                assert (want["status"][[0, 2]] & STATUS_DEPTH_INDEX).all()      # nearly every keypoint lies outside a 64x48 image
            elif name == "barrel" and flags == 1:
                # the undistorted-index flag on the barrel camera: the keypoints that left the image get no depth and status bit 0
                for f in (0, 2):
                    k = int(n[f])
                    ux, uy = got["kps_un"]["x"][f, :k], got["kps_un"]["y"][f, :k]
                    out = ~((ux > -1) & (ux < 752) & (uy > -1) & (uy < 480))
                    assert out.sum() > 10 and got["status"][f] & STATUS_DEPTH_INDEX
                    assert (got["depth"][f, :k][out] == -1).all() and (got["right_x"][f, :k][out] == -1).all()
            else:
                assert (want["depth"][0, :300] > 0).sum() > 100                 # depth was found
                if flags == 0:
                    assert not want["status"].any()
        return
    depth = None
    if source == "samples":
        rng = np.random.default_rng(5)
        depth = rng.uniform(0.3, 9.0, (3, fs.CAP)).astype(f32)
        depth[rng.uniform(size=depth.shape) < 0.2] = 0.0
        depth[0, 7], depth[0, 8] = np.nan, -3.0
    got, want, kps, n = _run_both(name, source, flags, depth)
    if source == "none":
        assert (got["depth"][0, :300] == -1).all() and (got["right_x"][2] == -1).all()
    assert got["status"][1] == 0 and got["cell_start"][1, -1] == 0              # the empty frame


def test_outputs_are_optional():
    from ydorbslam_amd.frame import frame_tail
    name = "tum_fr1"
    c, (w, h) = fs.cam(name), fs.size(name)
    kps, n = fs.batch(name)
    bounds = fs.ref_bounds(c, w, h)
    want = fs.ref_tail(c, kps, n, bounds=bounds)
    for w_ in (("grid",), ("kps_un",), ("right_x", "status"), ("depth",)):
        got = frame_tail(c, kps, n, bounds=bounds, want=w_)
        assert [k for k in ("kps_un", "right_x", "depth", "status") if got[k] is not None] == [k for k in ("kps_un", "right_x", "depth", "status") if k in w_]
        fs.same_tail(got, want, n)


@pytest.mark.parametrize("name", sorted(fs.CAMERAS))
def test_undistort_points_and_bounds(name):
    from ydorbslam_amd.frame import image_bounds, undistort_points
    c, (w, h) = fs.cam(name), fs.size(name)
    xy = fs.points(name, 1000)
    for n in (1, 63, 64, 65, 1000):
        assert np.array_equal(fs.bits(undistort_points(c, xy[:n])), fs.bits(fs.ref_undistort(c, xy[:n])[0])), n
    assert len(undistort_points(c, xy[:0])) == 0
    assert np.array_equal(fs.bits(image_bounds(c, w, h)), fs.bits(fs.ref_bounds(c, w, h)))


def test_negative_icdist_on_the_gpu():
    from ydorbslam_amd.frame import STATUS_ICDIST, camera, frame_tail, undistort_points
    c = camera(fs.TUM_K, (-10.0, 0.0, 0.0, 0.0, 0.0))
    xy = np.array([[18.0, 255.0], [320.0, 256.0], [600.0, 20.0]], f32)
    want, st = fs.ref_undistort(c, xy)
    assert st == STATUS_ICDIST and np.array_equal(fs.bits(undistort_points(c, xy)), fs.bits(want))
    kps = fs.keypoints(xy).reshape(1, -1)
    got = frame_tail(c, kps, [3], want=("kps_un", "status"))
    fs.same_tail(got, fs.ref_tail(c, kps, [3]), [3])
    assert got["status"][0] == STATUS_ICDIST


def test_grid_csr_cases():
    from ydorbslam_amd.frame import GRID_CELLS, frame_tail
    name = "barrel"
    c, (w, h) = fs.cam(name), fs.size(name)
    bounds = fs.ref_bounds(c, w, h)
    cap = 600
    rng = np.random.default_rng(9)
    # all in one cell: a cluster 0.05 px wide round the raw point (400 + k, 200) whose undistorted image lies nearest a cell's middle
    cand = np.array([[400.0 + k, 200.0] for k in range(16)], f32)
    un = fs.ref_undistort(c, cand)[0]
    gx, gy = (un[:, 0] - bounds[0]) * (64 / (bounds[1] - bounds[0])), (un[:, 1] - bounds[0]) * (48 / (bounds[3] - bounds[2]))
    mid = cand[np.argmin(np.maximum(np.abs(gx - np.rint(gx)), np.abs(gy - np.rint(gy))))]
    one = (mid + rng.uniform(0.0, 0.05, (cap, 2))).astype(f32)
    spread = fs.points(name, cap, seed=4)                                                                    # n = cap, some outside the grid
    kps = np.stack([fs.keypoints(one), fs.keypoints(spread), fs.keypoints(spread)])
    n = np.array([cap, cap, 0], np.int32)
    got, want = frame_tail(c, kps, n, bounds=bounds, want=("grid",)), fs.ref_tail(c, kps, n, bounds=bounds)
    fs.same_tail(got, want, n)
    cs, ci = got["cell_start"], got["cell_idx"]
    assert cs.shape == (3, GRID_CELLS + 1)
    assert (np.diff(cs[0]) > 0).sum() == 1 and cs[0, -1] == cap and np.array_equal(ci[0], np.arange(cap))
    assert 0 < cs[1, -1] < cap                                                   # the keypoints outside the grid are left out
    for cell, idx in fs.csr_lists(cs[1], ci[1]).items():
        assert idx == sorted(idx), cell                                          # ascending inside every cell
    assert not cs[2].any()


def _chain_camera():
    from ydorbslam_amd.frame import camera
    return camera((229.3, 228.6, 160.4, 119.7), fs.CAMERAS["barrel"][1])


def test_device_chain_behind_extractor_and_in_front_of_matcher():
    """extract_batch_device -> frame tail (device pointers) -> match_consecutive_device on one stream, nothing synchronised in between."""
    import torch
    import ydorbslam_amd as y
    from ydorbslam_amd.frame import DEPTH_U16, GRID_CELLS, frame_tail, frame_tail_device, image_bounds
    from ydorbslam_amd.synth import synth_frame
    F, W, H = 4, 320, 240
    imgs = np.stack([synth_frame(W, H, 40 + i) for i in range(F)])
    c = _chain_camera()
    bounds = image_bounds(c, W, H)
    depth = fs.depth_images((W, H), seed=8)[0][:3]
    depth = np.concatenate([depth, depth[:1]])                                   # [4, H, W] uint16
    ex = y.OrbExtractor(500, max_batch=F)
    cap = ex.max_keypoints
    dev = torch.device("cuda:0")
    d_img, d_depth = torch.from_numpy(imgs).to(dev), torch.from_numpy(depth.view(np.int16)).to(dev)
    d_kps = torch.zeros((F, cap, 7), dtype=torch.float32, device=dev)
    d_un = torch.zeros((F, cap, 7), dtype=torch.float32, device=dev)
    d_desc = torch.zeros((F, cap, 32), dtype=torch.uint8, device=dev)
    d_n = torch.zeros(F, dtype=torch.int32, device=dev)
    d_rx, d_dz = (torch.zeros((F, cap), dtype=torch.float32, device=dev) for _ in range(2))
    d_cs = torch.zeros((F, GRID_CELLS + 1), dtype=torch.int32, device=dev)
    d_ci = torch.zeros((F, cap), dtype=torch.int32, device=dev)
    d_st = torch.full((F,), 99, dtype=torch.int32, device=dev)
    d_asg = torch.zeros((F - 1, cap), dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(F - 1, dtype=torch.int32, device=dev)
    m = y.OrbMatcher(0.9, True)
    sf = ex.tables()["scale"]
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    ex.extract_batch_device(d_img.data_ptr(), W, H, W, W * H, F, d_kps.data_ptr(), d_desc.data_ptr(), cap, d_n.data_ptr(), stream=s.cuda_stream)
    frame_tail_device(c, d_kps.data_ptr(), d_n.data_ptr(), F, cap, d_un.data_ptr(), d_rx.data_ptr(), d_dz.data_ptr(), d_cs.data_ptr(), d_ci.data_ptr(),
                      d_st.data_ptr(), d_depth.data_ptr(), DEPTH_U16, W, H, 2 * W, 2 * W * H, FACTOR, fs.BF, bounds, stream=s.cuda_stream)
    m.match_consecutive_device(d_un.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), cap, F, W, H, 15.0, sf, d_asg.data_ptr(), d_cnt.data_ptr(),
                               stream=s.cuda_stream)
    s.synchronize()
    ex.synchronize()
    n = d_n.cpu().numpy()
    assert (n > 100).all()

    def kp(t):
        return t.cpu().numpy().view(np.uint8).reshape(F, cap, 28).view(y.KP_DTYPE).reshape(F, cap)
    raw = kp(d_kps)
    dev_out = dict(kps_un=kp(d_un), right_x=d_rx.cpu().numpy(), depth=d_dz.cpu().numpy(), cell_start=d_cs.cpu().numpy(), cell_idx=d_ci.cpu().numpy(),
                   status=d_st.cpu().numpy())
    kw = dict(depth=depth, factor=FACTOR, bf=fs.BF, bounds=bounds)
    host = frame_tail(c, raw, n, **kw)
    fs.same_tail(dev_out, host, n)
    want = fs.ref_tail(c, raw, n, **kw)
    fs.same_tail(host, want, n)
    assert (want["depth"][0, :n[0]] > 0).sum() > 50 and np.abs(want["kps_un"]["x"][0, :n[0]] - raw["x"][0, :n[0]]).max() > 1.0
    # the matcher on the restatement's undistorted keypoints gives the chain's assignments
    un = np.zeros((F, cap), y.KP_DTYPE)
    for f in range(F):
        un[f, :n[f]] = want["kps_un"][f, :n[f]]
    d_un2 = torch.from_numpy(un.view(np.float32).reshape(F, cap, 7)).to(dev)
    d_asg2, d_cnt2 = torch.zeros_like(d_asg), torch.zeros_like(d_cnt)
    m.match_consecutive_device(d_un2.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), cap, F, W, H, 15.0, sf, d_asg2.data_ptr(), d_cnt2.data_ptr())
    m.synchronize()
    cnt = d_cnt.cpu().numpy()
    assert np.array_equal(cnt, d_cnt2.cpu().numpy()) and (cnt > 20).all()
    a, a2 = d_asg.cpu().numpy(), d_asg2.cpu().numpy()
    for f in range(F - 1):
        assert np.array_equal(a[f, :n[f + 1]], a2[f, :n[f + 1]])
    # the device form without a keypoint output still builds the grid (scratch keypoints)
    d_cs2, d_ci2 = torch.zeros_like(d_cs), torch.zeros_like(d_ci)
    frame_tail_device(c, d_kps.data_ptr(), d_n.data_ptr(), F, cap, d_cell_start=d_cs2.data_ptr(), d_cell_idx=d_ci2.data_ptr(), bounds=bounds,
                      stream=s.cuda_stream)
    s.synchronize()
    assert torch.equal(d_cs, d_cs2)
    for f in range(F):
        assert torch.equal(d_ci[f, :d_cs[f, -1]], d_ci2[f, :d_cs[f, -1]])
    m.close()
    ex.close()


@pytest.mark.parametrize("with_depth", [True, False])
def test_extract_rgbd_equals_extract_plus_restatement(with_depth):
    import ydorbslam_amd as y
    from ydorbslam_amd.frame import extract_rgbd, image_bounds
    from ydorbslam_amd.synth import synth_frame
    W, H = 320, 240
    c = _chain_camera()
    bounds = image_bounds(c, W, H)
    big = np.zeros((H, W + 32), np.uint8)
    big[:, :W] = synth_frame(W, H, 44)
    gray = big[:, :W]                                                            # a stride above the width
    depth = fs.padded(fs.depth_images((W, H), seed=8)[0])[0] if with_depth else None
    ex = y.OrbExtractor(500)
    for _ in range(2):                                                           # the first call of a handle, and one on its warm plan
        got = extract_rgbd(ex, gray, depth, c, fs.BF, bounds, factor=FACTOR)
        kps, desc = ex.extract(np.ascontiguousarray(gray))
        n = len(kps)
        assert n > 100 and len(got["kps_raw"]) == n
        fs.same_keypoints(got["kps_raw"], kps)
        assert np.array_equal(got["desc"], desc)
        want = fs.ref_tail(c, kps.reshape(1, n), [n], depth=None if depth is None else depth[None], factor=FACTOR, bf=fs.BF, bounds=bounds)
        g = dict(kps_un=got["kps_un"][None], right_x=got["right_x"][None], depth=got["depth"][None], cell_start=got["cell_start"][None],
                 cell_idx=np.concatenate([got["cell_idx"], np.zeros(0, np.int32)])[None], status=np.array([got["status"]], np.int32))
        fs.same_tail(g, want, [n])
        if with_depth:
            assert (got["depth"] > 0).sum() > 50
        else:
            assert (got["depth"] == -1).all() and (got["right_x"] == -1).all()
    ex.close()


def test_arena_growth_and_release():
    from ydorbslam_amd.frame import frame_tail, release
    name = "tum_fr1"
    c, (w, h) = fs.cam(name), fs.size(name)
    bounds = fs.ref_bounds(c, w, h)
    release()
    small = fs.keypoints(fs.points(name, 40, seed=1)).reshape(1, 40)
    big = fs.keypoints(fs.points(name, 6 * 3000, seed=2)).reshape(6, 3000)
    nb = np.array([3000, 1, 2999, 0, 1500, 3000], np.int32)
    img = fs.depth_images((w, h))[1]
    img6 = np.concatenate([img, img])
    for kps, n, d in ((small, [40], img[:1]), (big, nb, img6), (small, [17], img[:1])):
        kw = dict(depth=d, bf=fs.BF, bounds=bounds)
        fs.same_tail(frame_tail(c, kps, n, **kw), fs.ref_tail(c, kps, n, **kw), n)
    release()
    kw = dict(depth=img[:1], bf=fs.BF, bounds=bounds)
    fs.same_tail(frame_tail(c, small, [40], **kw), fs.ref_tail(c, small, [40], **kw), [40])


def test_argument_errors():
    import ydorbslam_amd as y
    from ydorbslam_amd._lib import YdFrameTail
    from ydorbslam_amd.frame import DEPTH_F32, GRID_CELLS, camera, frame_tail, image_bounds, undistort_points
    L = y.lib()
    c = fs.cam("tum_fr1")
    kps = fs.keypoints(fs.points("tum_fr1", 8)).reshape(1, 8)
    img = np.ones((1, 480, 640), f32)

    def bad(fn, text):
        with pytest.raises(y.YdorbError, match=text):
            fn()
    bad(lambda: frame_tail(c, kps, [9], want=("kps_un",)), "outside 0..cap")                       # a count above cap
    bad(lambda: frame_tail(c, kps, [-1], want=("kps_un",)), "outside 0..cap")
    bad(lambda: frame_tail(camera(fs.TUM_K, (0.1, 0, 0, 0, 0), n_iter=0), kps, [8]), "n_iter")
    bad(lambda: undistort_points(camera(fs.TUM_K, n_iter=0), np.zeros((1, 2), f32)), "n_iter")
    bad(lambda: image_bounds(c, 0, 480), "size")
    bad(lambda: frame_tail(c, kps, [8], bounds=(0, 0, 0, 480)), "bounds")        # a grid over empty bounds

    def raw(**kw):
        T = YdFrameTail()
        n = np.array([8], np.int32)
        T.kps, T.n, T.n_frames, T.cap, T.cam = kps.ctypes.data, n.ctypes.data, 1, 8, c
        for k, v in kw.items():
            setattr(T, k, v)
        out = np.zeros(8, f32)
        rc = L.ydorb_frame_tail(C.byref(T), None, out.ctypes.data, None, None, None, None, None)
        assert rc == -1 and L.ydorb_last_error().decode().startswith("frame: "), (kw, rc)
    raw(kps=None)
    raw(n=None)
    raw(depth_type=DEPTH_F32, depth=None, depth_w=640, depth_h=480, depth_row_stride=2560)
    raw(depth_type=DEPTH_F32, depth=img.ctypes.data, depth_w=0, depth_h=480, depth_row_stride=2560)
    raw(depth_type=DEPTH_F32, depth=img.ctypes.data, depth_w=640, depth_h=-1, depth_row_stride=2560)
    raw(depth_type=DEPTH_F32, depth=img.ctypes.data, depth_w=640, depth_h=480, depth_row_stride=2559)   # a row stride below a row
    raw(depth_type=7)
    raw(n_frames=-1)
    raw(device=16)
    T = YdFrameTail()
    n = np.array([8], np.int32)
    T.kps, T.n, T.n_frames, T.cap, T.cam = kps.ctypes.data, n.ctypes.data, 1, 8, c
    cs = np.zeros(GRID_CELLS + 1, np.int32)
    assert L.ydorb_frame_tail(C.byref(T), None, None, None, cs.ctypes.data, None, None, None) == -1   # cell_start without cell_idx
    assert L.ydorb_frame_tail(None, None, None, None, None, None, None, None) == -1
    assert L.ydorb_undistort_points(C.byref(c), None, 3, None, 0) == -1 and L.ydorb_frame_release(99) == -1
    # ydorb_extract_rgbd: null handle, stride below the width, depth stride below a row
    ex = y.OrbExtractor(200)
    g = np.zeros((48, 64), np.uint8)
    k, d, nout = np.zeros(ex.max_keypoints, y.KP_DTYPE), np.zeros((ex.max_keypoints, 32), np.uint8), C.c_int32(5)
    args = lambda h, stride, dstride: (h, g.ctypes.data, 64, 48, stride, img.ctypes.data, DEPTH_F32, dstride, 1.0, C.byref(c), 1.0, None, 0,
                                       k.ctypes.data, None, d.ctypes.data, None, None, None, None, len(k), C.byref(nout), None)
    assert L.ydorb_extract_rgbd(*args(None, 64, 256)) == -1
    assert L.ydorb_extract_rgbd(*args(ex._h, 63, 256)) == -1
    assert L.ydorb_extract_rgbd(*args(ex._h, 64, 255)) == -1 and b"stride" in L.ydorb_last_error()
    ex.close()
