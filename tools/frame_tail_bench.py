"""Time of the RGB-D Frame constructor's tail (undistortKeyPoints, computeStereoFromRGBD, assignKeyPointsToGrid) at the C entry points,
beside the test restatement (tests/frame_ref) on one CPU thread, TUM fr1 camera, 640x480 uint16 depth:
  (a) one_frame   ydorb_frame_tail, host form, 1 frame x 1000 keypoints: the depth image passed, and per-keypoint samples passed;
  (b) batch       the same for 256 frames x 1000 keypoints in one call;
  (c) chain       device-resident, 512 frames on one stream: ydorb_extract_batch_device alone against extract + tail (device
                  pointers), every timing ending in a stream synchronise;
  (d) rgbd        ydorb_extract_rgbd (one call, one read-back) against ydorb_extract followed by the restatement of the tail on
                  the host, which is what the per-frame drop-in does without this entry.
Median wall time after warm-up with [min, max] of the repetitions.  Before and after timing all outputs are compared with the
restatement bit for bit.  Prints one JSON line."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import frame_support as S  # noqa: E402
import ydorbslam_amd as y  # noqa: E402
from ydorbslam_amd._lib import YdFrameTail  # noqa: E402
from ydorbslam_amd.frame import DEPTH_SAMPLES, DEPTH_U16, GRID_CELLS, extract_rgbd, frame_tail_device  # noqa: E402
from ydorbslam_amd.synth import synth_frame  # noqa: E402

NAME, W, H = "tum_fr1", 640, 480
FACTOR = float(np.float32(1.0) / np.float32(5000.0))
p = lambda a: a.ctypes.data_as(C.c_void_p)


def times(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return [round(float(v) * 1e3, 4) for v in (np.median(ts), min(ts), max(ts))]


def outputs(F, cap):
    return dict(kps_un=np.zeros((F, cap), y.KP_DTYPE), right_x=np.zeros((F, cap), np.float32), depth=np.zeros((F, cap), np.float32),
                cell_start=np.zeros((F, GRID_CELLS + 1), np.int32), cell_idx=np.zeros((F, cap), np.int32), status=np.zeros(F, np.int32))


def tail_case(L, R, cam, bounds, F, n_kp, reps):
    """ydorb_frame_tail's host form against the restatement; the image form reads one depth image per frame."""
    kps = S.keypoints(S.points(NAME, F * n_kp, seed=F)).reshape(F, n_kp)
    n = np.full(F, n_kp, np.int32)
    img = np.ascontiguousarray(np.broadcast_to(S.depth_images((W, H))[0][:1], (F, H, W)))
    raw = img[np.arange(F)[:, None], kps["y"].astype(np.int32), kps["x"].astype(np.int32)]
    samples = np.ascontiguousarray(raw.astype(np.float32) * np.float32(FACTOR))
    res = {}
    for form, depth, dtype in (("image", img, DEPTH_U16), ("samples", samples, DEPTH_SAMPLES)):
        T = YdFrameTail()
        T.kps, T.n, T.n_frames, T.cap, T.cam, T.bf, T.depth, T.depth_type = p(kps), p(n), F, n_kp, cam, S.BF, depth.ctypes.data, dtype
        T.depth_factor = FACTOR
        T.bounds[:] = [float(b) for b in bounds]
        if form == "image":
            T.depth_w, T.depth_h, T.depth_row_stride, T.depth_frame_stride = W, H, img.strides[1], img.strides[0]
        g, c = outputs(F, n_kp), outputs(F, n_kp)
        args = lambda o: (C.byref(T), p(o["kps_un"]), p(o["right_x"]), p(o["depth"]), p(o["cell_start"]), p(o["cell_idx"]), p(o["status"]))
        gpu = lambda: L.ydorb_frame_tail(*args(g), None)
        cpu = lambda: R.frameref_frame_tail(*args(c))
        if gpu() != 0:
            raise SystemExit("ydorb_frame_tail failed: " + L.ydorb_last_error().decode())
        cpu()
        S.same_tail(g, c, n)
        for _ in range(3):
            gpu()
        res[form] = dict(gpu_ms=times(gpu, reps), cpu_ms=times(cpu, max(reps // 3, 3)))
        g["kps_un"][:], g["right_x"][:], g["cell_start"][:] = 0, 0, -1
        assert gpu() == 0
        S.same_tail(g, c, n)
    both = dict(depth_found=int((c["depth"] > 0).sum()))
    both.update(res)
    return both


def chain_case(cam, bounds, F, reps):
    import torch
    dev = torch.device("cuda:0")
    base = np.stack([synth_frame(W, H, 500 + i) for i in range(8)])
    imgs = np.ascontiguousarray(np.tile(base, (F // 8, 1, 1)))
    depth = S.depth_images((W, H))[0][:1]
    ex = y.OrbExtractor(1000, max_batch=F)
    cap = ex.max_keypoints
    d_img, d_depth = torch.from_numpy(imgs).to(dev), torch.from_numpy(depth.view(np.int16)).to(dev)
    d_kps, d_un = (torch.zeros((F, cap, 7), dtype=torch.float32, device=dev) for _ in range(2))
    d_desc = torch.zeros((F, cap, 32), dtype=torch.uint8, device=dev)
    d_n, d_st = (torch.zeros(F, dtype=torch.int32, device=dev) for _ in range(2))
    d_rx, d_dz = (torch.zeros((F, cap), dtype=torch.float32, device=dev) for _ in range(2))
    d_cs = torch.zeros((F, GRID_CELLS + 1), dtype=torch.int32, device=dev)
    d_ci = torch.zeros((F, cap), dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(device=dev)

    def extract():
        ex.extract_batch_device(d_img.data_ptr(), W, H, W, W * H, F, d_kps.data_ptr(), d_desc.data_ptr(), cap, d_n.data_ptr(), stream=s.cuda_stream)

    def alone():
        extract()
        s.synchronize()

    def chained():
        extract()
        frame_tail_device(cam, d_kps.data_ptr(), d_n.data_ptr(), F, cap, d_un.data_ptr(), d_rx.data_ptr(), d_dz.data_ptr(), d_cs.data_ptr(),
                          d_ci.data_ptr(), d_st.data_ptr(), d_depth.data_ptr(), DEPTH_U16, W, H, 2 * W, 0, FACTOR, S.BF, bounds, stream=s.cuda_stream)
        s.synchronize()

    def check():
        chained()
        n = d_n.cpu().numpy()
        kp = lambda t: t.cpu().numpy().view(np.uint8).reshape(F, cap, 28).view(y.KP_DTYPE).reshape(F, cap)
        got = dict(kps_un=kp(d_un), right_x=d_rx.cpu().numpy(), depth=d_dz.cpu().numpy(), cell_start=d_cs.cpu().numpy(), cell_idx=d_ci.cpu().numpy(),
                   status=d_st.cpu().numpy())
        want = S.ref_tail(cam, kp(d_kps), n, depth=np.broadcast_to(depth, (F, H, W)), factor=FACTOR, bf=S.BF, bounds=bounds)
        S.same_tail(got, want, n)
        return int(n.sum())

    total = check()
    for _ in range(3):
        alone(); chained()
    out = dict(frames=F, keypoints=total, extract_ms=times(alone, reps), extract_tail_ms=times(chained, reps))
    check()
    ex.synchronize()
    ex.close()
    return out


def rgbd_case(L, R, cam, bounds, reps):
    gray = synth_frame(W, H, 500)
    depth = S.depth_images((W, H))[0][0]
    ex = y.OrbExtractor(1000)
    kps, desc = ex.extract(gray)
    n = len(kps)

    def tail_on_host(k):
        return S.ref_tail(cam, k.reshape(1, -1), [len(k)], depth=depth[None], factor=FACTOR, bf=S.BF, bounds=bounds)

    def one_call():
        return extract_rgbd(ex, gray, depth, cam, S.BF, bounds, factor=FACTOR)

    def today():
        k, _ = ex.extract(gray)
        return tail_on_host(k)

    def check():
        got, want = one_call(), tail_on_host(kps)
        S.same_keypoints(got["kps_raw"], kps)
        assert np.array_equal(got["desc"], desc)
        g = dict(kps_un=got["kps_un"][None], right_x=got["right_x"][None], depth=got["depth"][None], cell_start=got["cell_start"][None],
                 cell_idx=got["cell_idx"][None], status=np.array([got["status"]], np.int32))
        S.same_tail(g, want, [n])

    check()
    for _ in range(5):
        one_call(); today()
    out = dict(keypoints=n, extract_rgbd_ms=times(one_call, reps), extract_then_host_tail_ms=times(today, reps), extract_ms=times(lambda: ex.extract(gray), reps),
               host_tail_ms=times(lambda: tail_on_host(kps), reps))
    check()
    ex.close()
    return out


def main():
    L, R = y.lib(), S.ref()
    cam = S.cam(NAME)
    bounds = S.ref_bounds(cam, W, H)
    out = {"metric": "frame_tail_ms", "camera": NAME, "one_frame": tail_case(L, R, cam, bounds, 1, 1000, 100),
           "batch": tail_case(L, R, cam, bounds, 256, 1000, 10), "chain": chain_case(cam, bounds, 512, 10), "rgbd": rgbd_case(L, R, cam, bounds, 50)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
