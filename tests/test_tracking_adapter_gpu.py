"""The C++ adapter include/ydorb/tracking.hpp (searchLocalPointsImpl) EXECUTED on the GPU (tests/cpp_host/tracking_run.cpp on stand-ins
of Frame / MapPoint that carry data): the first loop over the frame's own points, the skip flags, one ydorb_search_local_points call,
the write-back and the assignment equal a Python replay on the ctypes path: the track fields bit for bit, the visibility counters, the
last-seen frame ids and the frame's map-point slots."""
import os
import subprocess

import numpy as np
import pytest

import frustum_support as S
from frustum_support import ROOT, f32

pytestmark = pytest.mark.gpu
SRC = os.path.join(ROOT, "tests", "cpp_host", "tracking_run.cpp")
TH, RATIO, FRAME_ID = 3.0, 0.8, 41
REC = np.dtype([("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("view_cos", "<f4"), ("level", "<i4"), ("in_view", "<i4"), ("visible", "<i4"),
                ("last_seen", "<i4")])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("trk") / "tracking_run")
    lib_dir = os.path.join(ROOT, "ydorbslam_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpu_harness", "mockrt"),
                           "-I" + os.path.join(ROOT, "include"), SRC, "-o", out, "-L" + lib_dir, "-l:libydorb.so", "-Wl,-rpath," + lib_dir])
    return out


def _scenario():
    """frustum_support.local_map() as objects: the 300 local points, then one held point per keypoint the scenario marks taken, then one
    bad point.  The frame holds the held points in their keypoints' slots, the bad point in a free slot and, in another free slot, a
    local point that the reference side sees in view (matched earlier in this frame).  Skip-flagged local points are bad."""
    s = S.local_map()
    want = S.ref_search_local_points(s, TH, RATIO)
    t, n_kp, n_loc = s["table"], len(s["kps"]), s["table"].n
    rng = np.random.default_rng(3)
    taken_kp = np.nonzero(s["taken"])[0]
    n_all = n_loc + len(taken_kp) + 1
    pts = dict(pos=np.zeros((n_all, 3), f32), normal=np.zeros((n_all, 3), f32), min=np.ones(n_all, f32), max=np.full(n_all, 2, f32),
               desc=rng.integers(0, 256, (n_all, 32), dtype=np.uint8), bad=np.zeros(n_all, np.int32), n_obs=np.full(n_all, 3, np.int32),
               last_seen=rng.integers(0, FRAME_ID, n_all).astype(np.int32), visible=rng.integers(1, 50, n_all).astype(np.int32))
    pts["pos"][:n_loc], pts["normal"][:n_loc], pts["desc"][:n_loc] = t.pos_min[:, :3], t.normal_max[:, :3], t.desc
    # the stand-in's invariance getters multiply the raw distances by 0.8f / 1.2f, as the reference's do
    pts["max"][:n_loc] = t.max_distance
    pts["min"][:n_loc] = (t.max_distance / S.scale_factors()[7]).astype(f32)
    assert np.array_equal(f32(0.8) * pts["min"][:n_loc], t.pos_min[:, 3]) and np.array_equal(f32(1.2) * pts["max"][:n_loc], t.normal_max[:, 3])
    pts["n_obs"][:n_loc] = np.where(s["has_obs"] != 0, 2, 0)
    pts["bad"][:n_loc] = s["skip"]
    pts["bad"][n_all - 1] = 1
    slot = np.full(n_kp, -1, np.int32)
    slot[taken_kp] = n_loc + np.arange(len(taken_kp))
    free = np.nonzero(slot < 0)[0]
    matched_kps = set(np.nonzero(want["assigned"] >= 0)[0].tolist())
    free = [int(k) for k in free if k not in matched_kps]
    held_local = int(np.nonzero((want["status"] == 0) & (s["has_obs"] != 0))[0][5])
    slot[free[0]], slot[free[1]] = n_all - 1, held_local
    return dict(s=s, pts=pts, slot=slot, n_loc=n_loc, n_all=n_all, held_local=held_local, bad_slot=free[0], held_slot=free[1])


def _blob(sc):
    s, p = sc["s"], sc["pts"]
    v = s["view"]
    T = np.eye(4, dtype=f32)
    T[:3, :3], T[:3, 3] = np.array(v.Rcw[:], f32).reshape(3, 3), np.array(v.tcw[:], f32)
    b = [np.array([v.fx, v.fy, v.cx, v.cy, v.bf, v.min_x, v.max_x, v.min_y, v.max_y], f32).tobytes(), np.array([8], np.int32).tobytes(),
         S.scale_factors().tobytes(), np.array([s["log"]], f32).tobytes(), np.array([FRAME_ID], np.int32).tobytes(),
         np.array([TH, RATIO], f32).tobytes(), T.tobytes(), np.array(v.Ow[:], f32).tobytes(), np.array([len(s["kps"])], np.int32).tobytes(),
         s["kps"].tobytes(), s["desc"].tobytes(), s["right_x"].tobytes(), np.array([sc["n_all"]], np.int32).tobytes()]
    for i in range(sc["n_all"]):
        b += [p["pos"][i].tobytes(), p["normal"][i].tobytes(), np.array([p["min"][i], p["max"][i]], f32).tobytes(), p["desc"][i].tobytes(),
              np.array([p["bad"][i], p["n_obs"][i], p["last_seen"][i], p["visible"][i]], np.int32).tobytes()]
    b += [sc["slot"].tobytes(), np.array([sc["n_loc"]], np.int32).tobytes(), np.arange(sc["n_loc"], dtype=np.int32).tobytes()]
    return b"".join(b)


def _replay(sc):
    """searchLocalPointsImpl on the ctypes path."""
    import ydorbslam_amd as y
    from ydorbslam_amd.frustum import search_local_points
    s, p, n_loc = sc["s"], sc["pts"], sc["n_loc"]
    rec = np.zeros(sc["n_all"], REC)
    for k in ("u", "v", "ur", "view_cos", "level"):
        rec[k] = -7
    rec["visible"], rec["last_seen"] = p["visible"], p["last_seen"]
    slot = sc["slot"].copy()
    for i in range(len(slot)):
        j = slot[i]
        if j < 0:
            continue
        if p["bad"][j]:
            slot[i] = -1
            continue
        rec["visible"][j] += 1
        rec["last_seen"][j] = FRAME_ID
    skip = ((rec["last_seen"][:n_loc] == FRAME_ID) | (p["bad"][:n_loc] != 0)).astype(np.uint8)
    taken = np.array([1 if j >= 0 and p["n_obs"][j] > 0 else 0 for j in slot], np.uint8)
    m = y.OrbMatcher(RATIO, check_orientation=False)
    r = search_local_points(m, y.FrameView(s["kps"], s["desc"], S.BOUNDS, s["right_x"]), s["view"], s["table"], skip, p["n_obs"][:n_loc] > 0, TH, taken)
    m.close()
    for i in range(n_loc):
        if r["status"][i] == 1:
            continue
        rec["in_view"][i] = int(r["status"][i] == 0)
        if r["status"][i] == 0:
            for k in ("u", "v", "ur", "view_cos", "level"):
                rec[k][i] = r["rows"][k][i]
            rec["visible"][i] += 1
    a = r["assigned"]
    slot[a >= 0] = a[a >= 0]
    return (r["n_matches"] if r["n_to_match"] > 0 else 0), rec, slot, r, skip


def test_search_local_points_adapter_equals_ctypes_replay(exe, tmp_path):
    sc = _scenario()
    matches, rec, slot, r, skip = _replay(sc)
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(inp, "wb").write(_blob(sc))
    subprocess.check_call([exe, inp, outp])
    raw = open(outp, "rb").read()
    assert len(raw) == 4 + REC.itemsize * sc["n_all"] + 4 * len(slot)
    got_matches = int(np.frombuffer(raw, np.int32, 1)[0])
    got = np.frombuffer(raw, REC, sc["n_all"], 4)
    got_slot = np.frombuffer(raw, np.int32, len(slot), 4 + REC.itemsize * sc["n_all"])
    assert got_matches == matches >= 50
    for k in ("u", "v", "ur", "view_cos"):
        assert np.array_equal(got[k].view(np.uint32), rec[k].view(np.uint32)), k
    for k in ("level", "in_view", "visible", "last_seen"):
        assert np.array_equal(got[k], rec[k]), k
    assert np.array_equal(got_slot, slot)
    # the bad point the frame held: its slot is reset, the point untouched
    bad = sc["n_all"] - 1
    assert got_slot[sc["bad_slot"]] == -1 and got["visible"][bad] == sc["pts"]["visible"][bad] and got["last_seen"][bad] == sc["pts"]["last_seen"][bad]
    # the local point already matched in this frame: skipped by the frustum test, counted visible once, still in its slot, matched nowhere else
    h = sc["held_local"]
    assert skip[h] == 1 and r["status"][h] == 1 and got["visible"][h] == sc["pts"]["visible"][h] + 1 and got["last_seen"][h] == FRAME_ID
    assert got_slot[sc["held_slot"]] == h and int((got_slot == h).sum()) == 1 and got["in_view"][h] == 0 and got["u"][h] == -7
    # in-view points were counted once more; out-of-view ones keep their stale track members
    loc = np.arange(sc["n_loc"])
    inv = loc[r["status"] == 0]
    assert len(inv) > 100 and np.array_equal(got["visible"][inv], sc["pts"]["visible"][inv] + 1)
    out = loc[r["status"] > 1]
    assert len(out) > 20 and np.all(got["u"][out] == -7) and np.all(got["in_view"][out] == 0)
