"""GPU parity: ydorb_stereo_matches (C ABI) vs oracle/stereo_oracle.cpp, the restatement of Frame::computeStereoMatches
(reference src/frame.cpp:362-477).  Bar: identical float bit patterns.  Parity unpinned (see the oracle's header).

The replay form (the serial `leftIdx` walk) runs as ONE launch per call for fewer than 8 pairs or at most 1024 keypoints, and in
slices that hand the lagging index from launch to launch otherwise.  The tests of the sliced path, all against the oracle:
  test_default_slicing_of_a_ragged_batch        12 pairs above 1024 keypoints, no environment variable: nL around the slice edge
  test_chosen_slices                            YDORB_STEREO_SLICE 37..40 (each wave writes the hand-over), 3 and 1, both candidate forms
  test_lagging_index_across_slice_boundaries    slice edges placed by the oracle's trace where the index lags and a step did not complete
  test_sliced_device_resident_form              the device-pointer form of the 12-pair batch
Every other test here takes the one-launch path."""
import numpy as np
import pytest

from ydorbslam_amd.synth import synth_stereo_pair

pytestmark = pytest.mark.gpu

BF, B = 40.0, 0.1


def _oracle_pair(oracle_lib, left, right, n_features, kl=None, dl=None, kr=None, dr=None, by_kp=False):
    from oracle.orb_oracle import OrbExtractorOracle
    el, er = OrbExtractorOracle(n_features), OrbExtractorOracle(n_features)
    okl, odl = el.extract(left)
    okr, odr = er.extract(right)
    lv_l, lv_r = [], []
    for l in range(8):
        w, h, _ = el.level_dims(l)
        lv_l.append(el.level_padded(l)[19:19 + h, 19:19 + w])
        lv_r.append(er.level_padded(l)[19:19 + h, 19:19 + w])
    t = el.tables()
    kl = okl if kl is None else kl
    dl = odl if dl is None else dl
    kr = okr if kr is None else kr
    dr = odr if dr is None else dr
    return (okl, odl, okr, odr), oracle_lib.stereo_matches(kl, dl, kr, dr, lv_l, lv_r, t["scale"], t["inv_scale"], BF, B, by_kp)


def _pad(items, cap, dtype, tail=()):
    out = np.zeros((len(items), cap) + tuple(tail), dtype)
    for i, a in enumerate(items):
        out[i, :len(a)] = a
    return out


@pytest.mark.parametrize("by_kp", [False, True])
def test_batched_pairs_match_the_oracle(oracle_lib, by_kp):
    import ydorbslam_amd as y
    nf, pairs = 800, 3
    imgs, per = [], []
    for p in range(pairs):
        left, right, _ = synth_stereo_pair(640, 480, p)
        imgs += [left, right]
        per.append((left, right))
    ex = y.OrbExtractor(nf, 1.2, 8, 20, 7, max_batch=2 * pairs)
    res = ex.extract_batch(np.stack(imgs))
    cap = max(len(k) for k, _ in res)
    kl = _pad([res[2 * p][0] for p in range(pairs)], cap, y.KP_DTYPE)
    dl = _pad([res[2 * p][1] for p in range(pairs)], cap, np.uint8, (32,))
    kr = _pad([res[2 * p + 1][0] for p in range(pairs)], cap, y.KP_DTYPE)
    dr = _pad([res[2 * p + 1][1] for p in range(pairs)], cap, np.uint8, (32,))
    nl = np.array([len(res[2 * p][0]) for p in range(pairs)], np.int32)
    nr = np.array([len(res[2 * p + 1][0]) for p in range(pairs)], np.int32)
    m = y.OrbMatcher()
    rx, depth, kept, status = m.stereo_matches(ex, ex, kl, dl, nl, kr, dr, nr, BF, B, index_by_keypoint=by_kp, left_frames=(0, 2), right_frames=(1, 2))
    total = 0
    for p in range(pairs):
        (okl, _, okr, _), (orx, odepth, okept, ostatus) = _oracle_pair(oracle_lib, per[p][0], per[p][1], nf, by_kp=by_kp)
        assert len(okl) == nl[p] and len(okr) == nr[p]
        assert kept[p] == okept and status[p] == ostatus == 0
        assert np.array_equal(rx[p, :nl[p]].view(np.uint32), orx.view(np.uint32)), p
        assert np.array_equal(depth[p, :nl[p]].view(np.uint32), odepth.view(np.uint32)), p
        assert np.all(depth[p, nl[p]:] == -1)
        total += okept
    assert total > (300 if by_kp else 3)


def test_two_extractors_and_undefined_cases_are_reported(oracle_lib):
    """Left and right pyramids from two handles (as the reference's two extractors); a left keypoint below the image and a best
    right keypoint 8 px from the left edge exercise the two situations the reference leaves undefined."""
    import ydorbslam_amd as y
    nf = 600
    left, right, _ = synth_stereo_pair(640, 480, 5)
    el, er = y.OrbExtractor(nf), y.OrbExtractor(nf)
    kl, dl = el.extract(left)
    kr, dr = er.extract(right)
    kl, kr = kl.copy(), kr.copy()
    lvl0 = np.flatnonzero((kl["octave"] == 0) & (kl["x"] > 60) & (kl["y"] > 30) & (kl["y"] < 440))
    a, c = int(lvl0[0]), int(lvl0[1])
    kl["y"][c] = 480.5                      # row index past the table
    fake = kr[:1].copy()
    fake["x"], fake["y"], fake["octave"] = 8.0, kl["y"][a], 0
    kr = np.concatenate([kr, fake])
    dr = np.concatenate([dr, dl[a:a + 1]])  # distance 0 to left keypoint a -> best right column at x = 8
    m = y.OrbMatcher()
    for by_kp in (True, False):
        rx, depth, kept, status = m.stereo_matches(el, er, kl[None], dl[None], [len(kl)], kr[None], dr[None], [len(kr)], BF, 0.05, index_by_keypoint=by_kp)
        from oracle.orb_oracle import OrbExtractorOracle
        ol, orr = OrbExtractorOracle(nf), OrbExtractorOracle(nf)
        ol.extract(left)
        orr.extract(right)
        lv_l = [ol.level_padded(l)[19:19 + ol.level_dims(l)[1], 19:19 + ol.level_dims(l)[0]] for l in range(8)]
        lv_r = [orr.level_padded(l)[19:19 + orr.level_dims(l)[1], 19:19 + orr.level_dims(l)[0]] for l in range(8)]
        t = ol.tables()
        orx, odepth, okept, ostatus = oracle_lib.stereo_matches(kl, dl, kr, dr, lv_l, lv_r, t["scale"], t["inv_scale"], BF, 0.05, by_kp)
        assert status[0] == ostatus and kept[0] == okept
        if by_kp:
            assert ostatus == 3
        assert np.array_equal(rx[0].view(np.uint32), orx.view(np.uint32))
        assert np.array_equal(depth[0].view(np.uint32), odepth.view(np.uint32))


def test_argument_checks():
    import ydorbslam_amd as y
    ex = y.OrbExtractor(300)
    m = y.OrbMatcher()
    k = np.zeros((1, 4), y.KP_DTYPE)
    d = np.zeros((1, 4, 32), np.uint8)
    with pytest.raises(y.YdorbError):   # no pyramid yet
        m.stereo_matches(ex, ex, k, d, [0], k, d, [0], BF, B)
    ex.extract(synth_stereo_pair(320, 240, 0)[0])
    with pytest.raises(y.YdorbError):   # frame outside the last call
        m.stereo_matches(ex, ex, k, d, [0], k, d, [0], BF, B, right_frames=(1, 1))
    rx, depth, kept, status = m.stereo_matches(ex, ex, k, d, [0], k, d, [0], BF, B)
    assert kept[0] == 0 and np.all(rx == -1) and np.all(depth == -1)


@pytest.mark.parametrize("w,h,nf", [(1241, 376, 2000), (752, 480, 1000)])
def test_baseline_stereo_configurations(oracle_lib, w, h, nf):
    """BASELINE.json configs 3 and 4 (KITTI-00-size and EuRoC-MH-size stereo): extraction of both images and the stereo
    association, bit-exact against the oracle in both index forms."""
    import ydorbslam_amd as y
    left, right, drow = synth_stereo_pair(w, h, 11)
    ex = y.OrbExtractor(nf, 1.2, 8, 20, 7, max_batch=2)
    (kl, dl), (kr, dr) = ex.extract_batch(np.stack([left, right]))
    m = y.OrbMatcher()
    for by_kp in (False, True):
        rx, depth, kept, status = m.stereo_matches(ex, ex, kl[None], dl[None], [len(kl)], kr[None], dr[None], [len(kr)], BF, B,
                                                   index_by_keypoint=by_kp, left_frames=(0, 1), right_frames=(1, 1))
        (okl, odl, okr, odr), (orx, odepth, okept, ostatus) = _oracle_pair(oracle_lib, left, right, nf, by_kp=by_kp)
        assert okl.tobytes() == kl.tobytes() and okr.tobytes() == kr.tobytes() and np.array_equal(odl, dl) and np.array_equal(odr, dr)
        assert kept[0] == okept and status[0] == ostatus == 0
        assert np.array_equal(rx[0].view(np.uint32), orx.view(np.uint32)) and np.array_equal(depth[0].view(np.uint32), odepth.view(np.uint32))
        if by_kp:
            ok = depth[0] > 0
            assert ok.sum() > 0.3 * len(kl)
            disp = kl["x"][ok] - rx[0][ok]
            assert np.mean(np.abs(disp - drow[kl["y"][ok].astype(int)]) < 1.5 * 1.2 ** kl["octave"][ok]) > 0.9


def test_index_chain_that_depends_on_the_descriptor_history(oracle_lib):
    """Every other left descriptor is noise and a third are copies of one right descriptor, so whether a keypoint reaches
    `leftIdx++` depends on which descriptor the lagging index hands it."""
    import ydorbslam_amd as y
    nf = 700
    rng = np.random.default_rng(3)
    pairs = []
    for p in range(2):
        left, right, _ = synth_stereo_pair(640, 480, 20 + p, disparities=(9, 9, 9))
        pairs.append((left, right))
    ex = y.OrbExtractor(nf, 1.2, 8, 20, 7, max_batch=4)
    res = ex.extract_batch(np.stack([im for pr in pairs for im in pr]))
    m = y.OrbMatcher()
    for p, (left, right) in enumerate(pairs):
        (kl, dl), (kr, dr) = res[2 * p], res[2 * p + 1]
        dl = dl.copy()
        dl[1::2] = rng.integers(0, 256, dl[1::2].shape, dtype=np.uint8)
        dl[::3] = dr[len(dr) // 2]
        _, (orx, odepth, okept, ostatus) = _oracle_pair(oracle_lib, left, right, nf, dl=dl)
        rx, depth, kept, status = m.stereo_matches(ex, ex, kl[None], dl[None], [len(kl)], kr[None], dr[None], [len(kr)], BF, B,
                                                   left_frames=(2 * p, 1), right_frames=(2 * p + 1, 1))
        assert kept[0] == okept and status[0] == ostatus
        assert np.array_equal(rx[0].view(np.uint32), orx.view(np.uint32)) and np.array_equal(depth[0].view(np.uint32), odepth.view(np.uint32))


def test_device_resident_form_equals_the_host_form():
    """extract_batch_device -> stereo with YDORB_STEREO_DEVICE_POINTERS: nothing leaves HBM between the two calls."""
    import torch
    import ydorbslam_amd as y
    pairs, W, H, nf = 3, 640, 480, 800
    imgs = np.stack([im for p in range(pairs) for im in synth_stereo_pair(W, H, 30 + p)[:2]])
    ex = y.OrbExtractor(nf, max_batch=2 * pairs)
    cap = ex.max_keypoints
    dev = torch.device("cuda:0")
    d_img = torch.from_numpy(imgs).to(dev)
    d_kps = torch.zeros((2 * pairs, cap, 7), dtype=torch.float32, device=dev)
    d_desc = torch.zeros((2 * pairs, cap, 32), dtype=torch.uint8, device=dev)
    d_n = torch.zeros(2 * pairs, dtype=torch.int32, device=dev)
    ex.extract_batch_device(d_img.data_ptr(), W, H, W, W * H, 2 * pairs, d_kps.data_ptr(), d_desc.data_ptr(), cap, d_n.data_ptr())
    ex.synchronize()
    # de-interleave on the device: the stereo call takes [pairs][cap] arrays per side
    kl, kr = d_kps[0::2].contiguous(), d_kps[1::2].contiguous()
    dl, dr = d_desc[0::2].contiguous(), d_desc[1::2].contiguous()
    nl, nr = d_n[0::2].contiguous(), d_n[1::2].contiguous()
    torch.cuda.synchronize()
    m = y.OrbMatcher()
    to_kp = lambda t: t.cpu().numpy().view(np.uint8).reshape(pairs, cap, 28).view(y.KP_DTYPE).reshape(pairs, cap)
    for by_kp in (False, True):
        d_rx = torch.zeros((pairs, cap), dtype=torch.float32, device=dev)
        d_depth = torch.zeros((pairs, cap), dtype=torch.float32, device=dev)
        d_kept = torch.zeros(pairs, dtype=torch.int32, device=dev)
        d_status = torch.full((pairs,), 7, dtype=torch.int32, device=dev)
        m.stereo_matches_device(ex, ex, kl.data_ptr(), dl.data_ptr(), nl.data_ptr(), cap, kr.data_ptr(), dr.data_ptr(), nr.data_ptr(), cap, pairs, BF, B,
                                d_rx.data_ptr(), d_depth.data_ptr(), d_kept.data_ptr(), d_status.data_ptr(), index_by_keypoint=by_kp,
                                left_frames=(0, 2), right_frames=(1, 2))
        m.synchronize()
        rx, depth, kept, status = m.stereo_matches(ex, ex, to_kp(kl), dl.cpu().numpy(), nl.cpu().numpy(), to_kp(kr), dr.cpu().numpy(), nr.cpu().numpy(),
                                                   BF, B, index_by_keypoint=by_kp, left_frames=(0, 2), right_frames=(1, 2))
        assert np.array_equal(d_rx.cpu().numpy().view(np.uint32), rx.view(np.uint32))
        assert np.array_equal(d_depth.cpu().numpy().view(np.uint32), depth.view(np.uint32))
        assert np.array_equal(d_kept.cpu().numpy(), kept) and np.array_equal(d_status.cpu().numpy(), status) and kept.sum() > 0


def test_replay_with_and_without_row_lists(oracle_lib, monkeypatch):
    """The replay kernel takes a row's candidates from an index of the right keypoints sorted by the first row of their band (LDS) or
    scans every right keypoint's band (YDORB_STEREO_NO_ROW_LISTS forces the second form).  Same bits either way."""
    import ydorbslam_amd as y
    left, right, _ = synth_stereo_pair(640, 480, 41)
    ex = y.OrbExtractor(1000, max_batch=2)
    (kl, dl), (kr, dr) = ex.extract_batch(np.stack([left, right]))
    args = (ex, ex, kl[None], dl[None], [len(kl)], kr[None], dr[None], [len(kr)], BF, B)
    a = y.OrbMatcher().stereo_matches(*args, left_frames=(0, 1), right_frames=(1, 1))
    monkeypatch.setenv("YDORB_STEREO_NO_ROW_LISTS", "1")
    b = y.OrbMatcher().stereo_matches(*args, left_frames=(0, 1), right_frames=(1, 1))
    monkeypatch.delenv("YDORB_STEREO_NO_ROW_LISTS")
    _, (orx, odepth, okept, ostatus) = _oracle_pair(oracle_lib, left, right, 1000)
    for got in (a, b):
        assert got[2][0] == okept and got[3][0] == ostatus
        assert np.array_equal(got[0][0].view(np.uint32), orx.view(np.uint32)) and np.array_equal(got[1][0].view(np.uint32), odepth.view(np.uint32))


def test_every_right_keypoint_on_the_top_level(oracle_lib):
    """Right keypoints that all claim the top level have the widest bands (17 rows each instead of ~8 on average): every row's window of the
    sorted index is then as long as it can get for this keypoint density.  Still the reference's result."""
    import ydorbslam_amd as y
    left, right, _ = synth_stereo_pair(640, 480, 43)
    ex = y.OrbExtractor(1000, max_batch=2)
    (kl, dl), (kr, dr) = ex.extract_batch(np.stack([left, right]))
    kr2 = kr.copy()
    kr2["octave"] = 7
    got = y.OrbMatcher().stereo_matches(ex, ex, kl[None], dl[None], [len(kl)], kr2[None], dr[None], [len(kr2)], BF, B, left_frames=(0, 1), right_frames=(1, 1))
    _, (orx, odepth, okept, ostatus) = _oracle_pair(oracle_lib, left, right, 1000, kl=kl, dl=dl, kr=kr2, dr=dr)
    assert got[2][0] == okept and got[3][0] == ostatus
    assert np.array_equal(got[0][0].view(np.uint32), orx.view(np.uint32)) and np.array_equal(got[1][0].view(np.uint32), odepth.view(np.uint32))


def test_right_keypoints_crowded_into_a_few_rows(oracle_lib):
    """More than 128 index entries in one row's window (the first trip of the candidate scan takes two per lane): the right keypoints are
    moved onto three image rows, the left ones onto the same rows, so every step walks several trips.  Same bits as the oracle and the scan form."""
    import ydorbslam_amd as y
    left, right, _ = synth_stereo_pair(640, 480, 44)
    ex = y.OrbExtractor(1000, max_batch=2)
    (kl, dl), (kr, dr) = ex.extract_batch(np.stack([left, right]))
    kl2, kr2 = kl.copy(), kr.copy()
    kr2["y"] = (200 + 40 * (np.arange(len(kr2)) % 3)).astype(np.float32) + (kr2["y"] - np.floor(kr2["y"]))
    kl2["y"] = (200 + 40 * (np.arange(len(kl2)) % 3)).astype(np.float32) + (kl2["y"] - np.floor(kl2["y"]))
    args = (ex, ex, kl2[None], dl[None], [len(kl2)], kr2[None], dr[None], [len(kr2)], BF, B)
    got = y.OrbMatcher().stereo_matches(*args, left_frames=(0, 1), right_frames=(1, 1))
    _, (orx, odepth, okept, ostatus) = _oracle_pair(oracle_lib, left, right, 1000, kl=kl2, dl=dl, kr=kr2, dr=dr)
    assert got[2][0] == okept and got[3][0] == ostatus
    assert np.array_equal(got[0][0].view(np.uint32), orx.view(np.uint32)) and np.array_equal(got[1][0].view(np.uint32), odepth.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------------
# The sliced replay.  A batch is several members over ONE extracted pyramid pair (frame step 0): keypoint and descriptor arrays are
# plain inputs to both sides, so members differ by truncation (ragged nL / nR) and by their left descriptors.
# ---------------------------------------------------------------------------------------------------------------------------------
REPLAY_WAVES = 4   # waves that share a pair's walk in k_stereo<true>: three steps are speculated ahead of the exact index


def _shared_scene(w, h, nf, index, disparities=(7, 15, 26), gpu=True):
    """One stereo pair: keypoints, descriptors and level images from the oracle extractor and, with gpu, the same pair extracted
    by a device extractor whose pyramids the stereo call reads (frames 0 and 1 of its last call)."""
    from oracle.orb_oracle import OrbExtractorOracle
    left, right, _ = synth_stereo_pair(w, h, index, disparities=disparities)
    el, er = OrbExtractorOracle(nf), OrbExtractorOracle(nf)
    kl, dl = el.extract(left)
    kr, dr = er.extract(right)
    lv_l = [el.level_padded(l)[19:19 + el.level_dims(l)[1], 19:19 + el.level_dims(l)[0]] for l in range(8)]
    lv_r = [er.level_padded(l)[19:19 + er.level_dims(l)[1], 19:19 + er.level_dims(l)[0]] for l in range(8)]
    t = el.tables()
    S = dict(kl=kl, dl=dl, kr=kr, dr=dr, lv_l=lv_l, lv_r=lv_r, scale=t["scale"], inv=t["inv_scale"], ex=None)
    if gpu:
        import ydorbslam_amd as y
        ex = y.OrbExtractor(nf, 1.2, 8, 20, 7, max_batch=2)
        (gkl, gdl), (gkr, gdr) = ex.extract_batch(np.stack([left, right]))
        assert gkl.tobytes() == kl.tobytes() and gkr.tobytes() == kr.tobytes() and np.array_equal(gdl, dl) and np.array_equal(gdr, dr)
        S["ex"] = ex
    return S


def _spoiled(S, seed):
    """Left descriptors of test_index_chain_that_depends_on_the_descriptor_history: every other row noise, every third a copy of one
    right descriptor - the index then falls behind the keypoint and the kernel's guesses of it fail."""
    rng = np.random.default_rng(seed)
    dl = S["dl"].copy()
    dl[1::2] = rng.integers(0, 256, dl[1::2].shape, dtype=np.uint8)
    dl[::3] = S["dr"][len(S["dr"]) // 2]
    return dl


def _oracle_members(oracle_lib, S, members):
    """members: list of (nL, nR, left descriptors [len(kl), 32]).  The oracle's (rx, depth, kept, status, s, complete) per member."""
    return [oracle_lib.stereo_matches_trace(S["kl"][:nl], dl[:nl], S["kr"][:nr], S["dr"][:nr], S["lv_l"], S["lv_r"], S["scale"], S["inv"], BF, B)
            for nl, nr, dl in members]


def _batch_arrays(S, members):
    """[members, cap] inputs: every member carries the FULL keypoint / descriptor arrays and only its counts say where it ends, so a
    kernel that walked past nL or nR would find real data there."""
    n = len(members)
    kl = np.ascontiguousarray(np.tile(S["kl"], (n, 1)))
    kr = np.ascontiguousarray(np.tile(S["kr"], (n, 1)))
    dl = np.ascontiguousarray(np.stack([m[2] for m in members]))
    dr = np.ascontiguousarray(np.tile(S["dr"], (n, 1, 1)))
    nl = np.array([m[0] for m in members], np.int32)
    nr = np.array([m[1] for m in members], np.int32)
    return kl, dl, nl, kr, dr, nr


def _assert_equals_oracle(got, ref, members, what=""):
    rx, depth, kept, status = got
    for p, ((nl, nr, _), (orx, odepth, okept, ostatus, _, _)) in enumerate(zip(members, ref)):
        assert kept[p] == okept and status[p] == ostatus, (what, p, nl, nr, int(kept[p]), okept, int(status[p]), ostatus)
        bad = np.flatnonzero((rx[p, :nl].view(np.uint32) != orx.view(np.uint32)) | (depth[p, :nl].view(np.uint32) != odepth.view(np.uint32)))
        assert len(bad) == 0, (what, p, nl, nr, "first differing output slots", bad[:8].tolist())
        assert np.all(rx[p, nl:] == -1) and np.all(depth[p, nl:] == -1), (what, p, "padding written")


def _run_host(S, members):
    import ydorbslam_amd as y
    kl, dl, nl, kr, dr, nr = _batch_arrays(S, members)
    return y.OrbMatcher().stereo_matches(S["ex"], S["ex"], kl, dl, nl, kr, dr, nr, BF, B, left_frames=(0, 0), right_frames=(1, 0))


def _kitti_members(S):
    """The ragged 12-member batch of the default-slicing tests (slice 1024): counts around the slice edge, natural and spoiled
    descriptors, short and empty right sides."""
    n, nr = len(S["kl"]), len(S["kr"])
    assert n > 1100 and nr > 1100, (n, nr)
    nat, sp1, sp2 = S["dl"], _spoiled(S, 5), _spoiled(S, 6)
    return [(n, nr, nat), (1024, nr, sp1), (1025, nr, sp1), (700, nr, nat), (0, nr, nat), (n, nr, sp1), (n - 3, 1200, sp2), (1026, nr, nat),
            (1023, nr, sp2), (n, 0, nat), (1, nr, nat), (1500, nr, sp2)]


@pytest.fixture(scope="module")
def kitti_scene(oracle_lib):
    """KITTI-size pair (BASELINE.json config 3): capacity above 1024, so 8 or more members are walked in slices of 1024."""
    S = _shared_scene(1241, 376, 2000, 11)
    S["members"] = _kitti_members(S)
    S["ref"] = _oracle_members(oracle_lib, S, S["members"])
    return S


def test_default_slicing_of_a_ragged_batch(oracle_lib, kitti_scene, monkeypatch):
    """12 members, capacity > 1024, no environment variable: the host cuts the walk at 1024.  nL == 1024 ends with the first slice
    (nothing handed over, the second launch returns at once), nL == 1025 leaves one step that wave 0 runs alone, nL above, below, 1, 0."""
    monkeypatch.delenv("YDORB_STEREO_SLICE", raising=False)
    monkeypatch.delenv("YDORB_STEREO_NO_ROW_LISTS", raising=False)
    S = kitti_scene
    members, ref = S["members"], S["ref"]
    nls = [m[0] for m in members]
    assert len(members) >= 8 and len(S["kl"]) > 1024
    assert sum(nl > 1025 for nl in nls) >= 3 and 1024 in nls and 1025 in nls and 0 in nls and any(0 < nl < 1024 for nl in nls)
    # the index really is handed over in different states: behind the keypoint for some members, level with it for none of the long ones
    lag = [1024 - int(r[4][1024]) for (nl, _, _), r in zip(members, ref) if nl > 1024]
    assert max(lag) > REPLAY_WAVES and sum(r[2] for r in ref) > 100, lag
    _assert_equals_oracle(_run_host(S, members), ref, members, "default slice")


@pytest.mark.parametrize("slice_len,no_lists", [(37, False), (38, False), (39, False), (40, False), (3, False), (39, True), (3, True)])
def test_chosen_slices(oracle_lib, slice_len, no_lists, monkeypatch):
    """YDORB_STEREO_SLICE per call.  The wave that ran the last step of a slice writes the hand-over: slices of 37, 38, 39 and 40 steps
    make that wave 0, 1, 2 and 3; in slices of 3 steps one wave never has a step.  Candidates from the row lists or the band scan."""
    S = _chosen_scene(oracle_lib)
    members, ref = S["members"], S["ref"]
    assert len(members) >= 2 and {(L - 1) % REPLAY_WAVES for L in (37, 38, 39, 40)} == set(range(REPLAY_WAVES)) and 3 < REPLAY_WAVES
    monkeypatch.setenv("YDORB_STEREO_SLICE", str(slice_len))
    if no_lists:
        monkeypatch.setenv("YDORB_STEREO_NO_ROW_LISTS", "1")
    else:
        monkeypatch.delenv("YDORB_STEREO_NO_ROW_LISTS", raising=False)
    _assert_equals_oracle(_run_host(S, members), ref, members, "slice %d" % slice_len)


_CHOSEN = {}


def _chosen_scene(oracle_lib):
    """640x480 / 800 features, three members: natural, spoiled and a spoiled one cut short (one extraction for every slice length)."""
    if not _CHOSEN:
        S = _shared_scene(640, 480, 800, 21, disparities=(9, 9, 9))
        n, nr = len(S["kl"]), len(S["kr"])
        S["members"] = [(n, nr, S["dl"]), (n, nr, _spoiled(S, 3)), (n - 150, nr - 40, _spoiled(S, 4))]
        S["ref"] = _oracle_members(oracle_lib, S, S["members"])
        _CHOSEN.update(S)
    return _CHOSEN


def test_slices_of_one_step(oracle_lib, monkeypatch):
    """Slice 1 on a small frame: every step reads the hand-over and writes it, wave 0 alone (a few hundred launches per call)."""
    S = _shared_scene(480, 360, 300, 22, disparities=(9, 9, 9))
    n, nr = len(S["kl"]), len(S["kr"])
    assert 100 < n < 600
    members = [(n, nr, S["dl"]), (n - 7, nr, _spoiled(S, 8))]
    ref = _oracle_members(oracle_lib, S, members)
    assert all(0 < r[5].sum() < len(r[5]) for r in ref)     # steps that complete and steps that do not
    monkeypatch.delenv("YDORB_STEREO_NO_ROW_LISTS", raising=False)
    monkeypatch.setenv("YDORB_STEREO_SLICE", "1")
    _assert_equals_oracle(_run_host(S, members), ref, members, "slice 1")


def _boundary_kinds(ref, members, slice_len):
    """Over the slice edges kBegin = slice_len, 2 * slice_len, ... < nL of every member, from the oracle's trace: how many follow a step
    that did not reach `leftIdx++`, how many follow one that did, and at how many the index is more than REPLAY_WAVES behind kBegin."""
    incomplete = complete = lagging = 0
    for (nl, _, _), r in zip(members, ref):
        s, c = r[4], r[5]
        for kb in range(slice_len, nl, slice_len):
            incomplete += int(c[kb - 1] == 0)
            complete += int(c[kb - 1] == 1)
            lagging += int(kb - int(s[kb]) > REPLAY_WAVES)
    return incomplete, complete, lagging


def _lagging_plan(oracle_lib, gpu=True):
    """Scene, members, oracle results and slice lengths of test_lagging_index_across_slice_boundaries: 37..40 and three lengths that put
    an edge right behind a step that did not complete, read off the oracle's trace of the spoiled member."""
    S = _shared_scene(640, 480, 700, 20, disparities=(9, 9, 9), gpu=gpu)
    n, nr = len(S["kl"]), len(S["kr"])
    members = [(n, nr, _spoiled(S, 3)), (n - 61, nr, _spoiled(S, 13))]
    ref = _oracle_members(oracle_lib, S, members)
    s, c = ref[0][4], ref[0][5]
    after_skip = [k + 1 for k in range(40, n - 1) if c[k] == 0 and (k + 1) - int(s[k + 1]) > REPLAY_WAVES]
    assert len(after_skip) >= 3, "the spoiled descriptors leave no incomplete step with a lagging index"
    slices = [37, 38, 39, 40] + [after_skip[0], after_skip[len(after_skip) // 2], after_skip[-1]]
    return S, members, ref, slices


def test_lagging_index_across_slice_boundaries(oracle_lib, monkeypatch):
    """Noise rows and copies of one right descriptor make the index fall behind the keypoint and the speculating waves' guesses fail.
    Checked on the oracle's trace before anything runs on the GPU: among the slice edges walked there is one behind a step that did not
    complete, one behind a step that did, and one where the index handed over is more than the wave count behind kBegin."""
    S, members, ref, slices = _lagging_plan(oracle_lib)
    totals = np.sum([_boundary_kinds(ref, members, L) for L in slices], axis=0)
    assert totals[0] >= 1 and totals[1] >= 1 and totals[2] >= 1, totals.tolist()
    for L in slices[4:]:                              # each of the placed edges has all three properties but `complete`
        k = _boundary_kinds(ref, members[:1], L)
        assert k[0] >= 1 and k[2] >= 1, (L, k)
    monkeypatch.delenv("YDORB_STEREO_NO_ROW_LISTS", raising=False)
    for L in slices:
        monkeypatch.setenv("YDORB_STEREO_SLICE", str(L))
        _assert_equals_oracle(_run_host(S, members), ref, members, "slice %d" % L)


def test_sliced_device_resident_form(oracle_lib, kitti_scene, monkeypatch):
    """The 12-member batch of test_default_slicing_of_a_ragged_batch through the device-pointer form: the same bits as the host form
    (and so the oracle's), default slices of 1024."""
    import torch
    import ydorbslam_amd as y
    monkeypatch.delenv("YDORB_STEREO_SLICE", raising=False)
    monkeypatch.delenv("YDORB_STEREO_NO_ROW_LISTS", raising=False)
    S = kitti_scene
    members, ref = S["members"], S["ref"]
    kl, dl, nl, kr, dr, nr = _batch_arrays(S, members)
    pairs, cap_l, cap_r = len(members), kl.shape[1], kr.shape[1]
    assert pairs >= 8 and cap_l > 1024
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
    d_kl, d_dl, d_nl, d_kr, d_dr, d_nr = up(kl), up(dl), up(nl), up(kr), up(dr), up(nr)
    d_rx = torch.zeros((pairs, cap_l), dtype=torch.float32, device=dev)
    d_depth = torch.zeros((pairs, cap_l), dtype=torch.float32, device=dev)
    d_kept = torch.zeros(pairs, dtype=torch.int32, device=dev)
    d_status = torch.full((pairs,), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    m = y.OrbMatcher()
    m.stereo_matches_device(S["ex"], S["ex"], d_kl.data_ptr(), d_dl.data_ptr(), d_nl.data_ptr(), cap_l, d_kr.data_ptr(), d_dr.data_ptr(), d_nr.data_ptr(),
                            cap_r, pairs, BF, B, d_rx.data_ptr(), d_depth.data_ptr(), d_kept.data_ptr(), d_status.data_ptr(),
                            left_frames=(0, 0), right_frames=(1, 0))
    m.synchronize()
    got = (d_rx.cpu().numpy(), d_depth.cpu().numpy(), d_kept.cpu().numpy(), d_status.cpu().numpy())
    host = _run_host(S, members)
    for a, b in zip(got, host):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    _assert_equals_oracle(got, ref, members, "device form")
