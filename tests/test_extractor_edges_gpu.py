"""GPU: the HIP extractor on the edge-case table of tests/extractor_edge_support.py, bit for bit against the CPU oracle at every stage
(padded levels, blur, FAST candidates, level keypoints with their angle bits, final keypoints, descriptors), and - so that a kernel and an
oracle that are wrong in the same way still fail - against the plain definitions of that module where they say what the output must be:
level-0 candidates = fast_corner_definition + nms_definition per cell, the lattice's candidates = the lattice, blurred levels =
blur_definition, angle-0 descriptors = brief_at_angle_zero.  tests/test_extractor_edges_cpu.py proves that the images reach the
branches they are here for.
"""
import functools

import numpy as np
import pytest

import extractor_edge_support as es
from extractor_edge_support import LATTICE_FEATURES, NARROW_OFFSETS, SHEET_OFFSETS, lattice_images, sheet

pytestmark = pytest.mark.gpu

BATCH_OFFSETS = SHEET_OFFSETS + ((5, 7),)


class _Ref:
    """The oracle's stages for one image, computed once and never changed."""

    def __init__(self, cfg, img):
        from oracle.orb_oracle import OrbExtractorOracle
        cpu = OrbExtractorOracle(*cfg)
        self.kps, self.desc = cpu.extract(img)
        n = cfg[2]
        self.dims = [cpu.level_dims(l)[:2] for l in range(n)]
        self.padded = [cpu.level_padded(l)[:, :self.dims[l][0] + 38] for l in range(n)]
        self.blurred = [cpu.level_blurred(l) for l in range(n)]
        self.cands = [cpu.level_candidates(l) for l in range(n)]
        self.level_kps = [cpu.level_keypoints(l) for l in range(n)]


@functools.lru_cache(maxsize=None)
def _sheet_ref(thr, offset, narrow=False):
    return _Ref((1000, 1.2, 8, thr, 7), sheet(thr, offset, narrow)[0])


def _same_kps(a, b):
    assert len(a) == len(b)
    for f in a.dtype.names:
        assert np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)), "field %s differs" % f


def _cand_list(c):
    return list(zip(c["x"].astype(int), c["y"].astype(int), c["response"].astype(int)))


def _stages_equal(gpu, res, ref, frame=0):
    """Every stage of frame `frame` of the handle's last call against the oracle; then every blurred level against blur_definition of
    the level the GPU itself holds (the oracle blurs only levels that kept a keypoint)."""
    for l, (w, h) in enumerate(ref.dims):
        assert gpu.level_dims(l, frame)[:2] == (w, h)
        level = gpu.read_level(l, frame)
        assert np.array_equal(level, ref.padded[l]), "pyramid level %d" % l
        blurred = gpu.debug_read(0, l, frame)
        if ref.blurred[l] is not None:
            assert np.array_equal(blurred, ref.blurred[l]), "blurred level %d" % l
        if w >= 4 and h >= 4:
            assert np.array_equal(blurred, es.blur_definition(level[19:19 + h, 19:19 + w])), "blurred level %d, definition" % l
        assert _cand_list(gpu.debug_read(1, l, frame)) == _cand_list(ref.cands[l]), "candidates level %d" % l
        _same_kps(gpu.debug_read(2, l, frame), ref.level_kps[l])
    _same_kps(res[0], ref.kps)
    assert np.array_equal(res[1], ref.desc)


def _extractor(cfg, monkeypatch=None, env=None, **kw):
    import ydorbslam_amd as y
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    gpu = y.OrbExtractor(*cfg, **kw)
    for k in (env or {}):
        monkeypatch.delenv(k)
    return gpu


@pytest.mark.parametrize("offset", SHEET_OFFSETS)
@pytest.mark.parametrize("thr", [20, 7])
def test_patch_sheet_single_frame(oracle_lib, thr, offset):
    img, _ = sheet(thr, offset)
    gpu = _extractor((1000, 1.2, 8, thr, 7))
    res = gpu.extract(img)
    _stages_equal(gpu, res, _sheet_ref(thr, offset))
    assert _cand_list(gpu.debug_read(1, 0)) == es.level_candidates_definition(img, thr)


@pytest.mark.parametrize("thr", [20, 7])
def test_patch_sheet_batch_of_twelve(oracle_lib, thr):
    """A handle for more than 8 frames: two FAST level groups, k_qt_fast per group, four keypoints per wave in the descriptor kernel."""
    offsets = BATCH_OFFSETS * 3
    gpu = _extractor((1000, 1.2, 8, thr, 7), max_batch=12)
    res = gpu.extract_batch(np.stack([sheet(thr, o)[0] for o in offsets]))
    for f, o in enumerate(offsets):
        ref = _sheet_ref(thr, o)
        _same_kps(res[f][0], ref.kps)
        assert np.array_equal(res[f][1], ref.desc), f
        for l in range(8):
            assert _cand_list(gpu.debug_read(1, l, f)) == _cand_list(ref.cands[l]), (f, l)
    for f in range(len(BATCH_OFFSETS)):
        assert _cand_list(gpu.debug_read(1, 0, f)) == es.level_candidates_definition(sheet(thr, offsets[f])[0], thr), f


@pytest.mark.parametrize("offset", NARROW_OFFSETS)
def test_narrow_sheet_one_wide_cell(oracle_lib, offset):
    """Level 0 is a single cell with a 37 x 25 band: one row of up to 64 lanes per step in stage A."""
    img, placed = sheet(20, offset, True)
    gpu = _extractor((1000, 1.2, 8, 20, 7))
    res = gpu.extract(img)
    _stages_equal(gpu, res, _sheet_ref(20, offset, True))
    got = _cand_list(gpu.debug_read(1, 0))
    assert got == es.level_candidates_definition(img, 20) and len(got) >= len(placed) // 2


@pytest.mark.parametrize("form", ["flat", "pass"])
def test_lattice_quadtree_of_ties(oracle_lib, monkeypatch, form):
    """Levels 0 and 1 of the period-6 lattices are nothing but ties, with 60 times as many candidates as the quota: every node's
    choice is tie order alone (k_qt_fast's qt_sort_front replay, or the pass kernel with YDORB_QT_PASS=1).  Twice on one handle: the
    second call runs with the quad-tree footprints retuned from the first."""
    named = lattice_images()
    names = list(named)
    cfg = (LATTICE_FEATURES, 1.2, 8, 20, 7)
    refs = [_Ref(cfg, named[n][0]) for n in names]
    gpu = _extractor(cfg, monkeypatch, {"YDORB_QT_PASS": "1"} if form == "pass" else None, max_batch=len(names))
    imgs = np.stack([named[n][0] for n in names])
    for call in range(2):
        res = gpu.extract_batch(imgs)
        for f, n in enumerate(names):
            _stages_equal(gpu, res[f], refs[f], f)
            pts = named[n][1]
            want = [] if n == "bars6" else sorted((x - es.EDGE, y - es.EDGE, 254) for x, y in pts.tolist())
            assert sorted(_cand_list(gpu.debug_read(1, 0, f))) == want, n
            for l in range(8):
                if form == "pass":
                    assert gpu.debug_read(3, l, f) == 1
                elif n in ("lattice6", "inverse6"):
                    assert gpu.debug_read(3, l, f) == 0, (n, l)     # k_qt_fast itself finished the unit


def _angle_zero_by_definition(gpu, res, frame):
    """The frame's level-0 keypoints whose angle bits are 0: descriptor = the unrotated pattern on the GPU's own blurred level."""
    blurred = gpu.debug_read(0, 0, frame)
    k, d = res
    zero = np.nonzero((k["octave"] == 0) & (k["angle"].view(np.uint32) == 0))[0]
    for i in zero:
        assert np.array_equal(es.brief_at_angle_zero(blurred, int(k["x"][i]), int(k["y"][i]))[0], d[i]), (frame, i)
    return len(zero)


@pytest.mark.parametrize("kpw", ["1", "4"])
def test_oriented_marks(oracle_lib, monkeypatch, kpw):
    """The marks and their two mirror images (every sign of the moments changes place) through k_orient_describe (one keypoint per
    wave) and k_orient_describe_n<4>; a single-frame call on the same handle first."""
    frames = es.mark_frames()
    cfg = (1000, 1.2, 8, 20, 7)
    refs = [_Ref(cfg, f) for f in frames]
    gpu = _extractor(cfg, monkeypatch, {"YDORB_DESC_KPW": kpw}, max_batch=len(frames))
    res = gpu.extract(frames[0])
    _stages_equal(gpu, res, refs[0])
    assert _angle_zero_by_definition(gpu, res, 0) >= 8
    res = gpu.extract_batch(np.stack(frames))
    for f in range(len(frames)):
        _stages_equal(gpu, res[f], refs[f], f)
        assert _angle_zero_by_definition(gpu, res[f], f) >= 8


def test_saturated_images(oracle_lib):
    """All-255, 0/255 checkerboards, stripes and full-range noise: one by one on a single-frame handle, then as one batch."""
    named = es.saturated_images()
    cfg = (500, 1.2, 8, 20, 7)
    refs = {n: _Ref(cfg, img) for n, img in named.items()}
    single = _extractor(cfg)
    for n, img in named.items():
        _stages_equal(single, single.extract(img), refs[n])
    batch = _extractor(cfg, max_batch=len(named))
    res = batch.extract_batch(np.stack(list(named.values())))
    for f, n in enumerate(named):
        _stages_equal(batch, res[f], refs[n], f)
