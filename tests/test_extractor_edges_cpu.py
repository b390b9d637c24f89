"""The extractor's edge-case table (tests/extractor_edge_support.py) on the CPU oracle and the plain definitions, no GPU: every image
must reach the branch of extract_kernels.hip.h it is here for, so that tests/test_extractor_edges_gpu.py cannot pass vacuously.
These are conditions on the inputs, not measurements: the builders were tuned until they held.

The last test is the mutation check: three wrong detectors / descriptors, each restated in a copy of the definition, and for each an
assert of this file that passes on the right definition and fails on the wrong one.
"""
import functools
import math

import numpy as np
import pytest

import extractor_edge_support as es


def _set(kps, dx=0):
    return sorted(zip(kps["x"].astype(int) + dx, kps["y"].astype(int) + dx, kps["response"].astype(int)))


def _kinds(img, thr):
    """Per pixel: corner score, and the stage-B classes: 1 = compass passes both ways and only the brighter arcs detect it, 2 = both ways
    and only the darker arcs, 3 = both ways and not a corner, 0 = compass passes one way; -1 = no compass survivor."""
    score = es.fast_corner_definition(img, thr)
    dark, bright = es.fast_arc_scores(img)
    cd, cb = es.compass_flags(img, thr)
    both = cd & cb
    kind = np.where(~(cd | cb), -1, np.where(~both, 0, np.where((bright >= thr) & (dark < thr), 1, np.where((dark >= thr) & (bright < thr), 2, 3))))
    return score, kind


def test_vector_definition_is_the_scalar_one():
    """fast_corner_definition (numpy, every pixel at once) against _fast_score_definition (Python scalars) on random rings."""
    rng = np.random.default_rng(7)
    hits = 0
    for _ in range(300):
        p = np.clip(128 + rng.integers(-40, 41) + rng.integers(-12, 13, (7, 7)), 0, 255).astype(np.uint8)
        if rng.random() < 0.8:
            k, n, sign = rng.integers(0, 16), rng.integers(7, 14), rng.choice([-1, 1])
            for j in range(n):
                dx, dy = es.CIRCLE[(k + j) % 16]
                p[3 + dy, 3 + dx] = np.clip(int(p[3, 3]) + sign * rng.integers(15, 60), 0, 255)
        d16 = [int(p[3, 3]) - int(p[3 + dy, 3 + dx]) for dx, dy in es.CIRCLE]
        ref = es._fast_score_definition(d16, 20)
        hits += ref is not None
        assert es.fast_corner_definition(p, 20)[3, 3] == (ref or 0)
    assert hits > 50


@pytest.mark.parametrize("thr", [20, 7])
def test_patch_sheet_reaches_both_arc_networks_and_the_value_range(oracle_lib, thr):
    img, placed = es.sheet(thr, (0, 0))
    assert len(placed) == len(es.patch_kinds(thr)) == 49 * 4 * 2 * 7 and img.shape[0] <= 480
    score, kind = _kinds(img, thr)
    # the definition's corner set is the oracle's, score for score, before NMS
    ys, xs = np.nonzero(score)
    assert sorted(zip(xs, ys, score[ys, xs])) == _set(oracle_lib.fast9_16(img, thr, nms=False))
    # every patch is what its row of the table says
    assert np.array_equal(score[placed["y"], placed["x"]] > 0, placed["corner"])
    assert (score[placed["y"], placed["x"]][placed["corner"]] == thr).all()
    assert (img[placed["y"], placed["x"]] == placed["centre"]).all()
    # stage B: pixels that only the second (brighter) network detects, and the mirror case
    corner = score > 0
    assert ((kind == 1) & corner).sum() >= 64 and ((kind == 2) & corner).sum() >= 64
    # ... and a full chunk of 64 consecutive compass survivors of one cell (row-major) that holds both with one-way pixels
    h, w = img.shape
    mixed = 0
    for (x0, y0, x1, y1) in es.bands_of_level(w, h):
        kk = kind[y0:y1, x0:x1]
        kk = kk[kk >= 0]                                        # boolean indexing is row-major
        for c in range(0, len(kk) - 63, 64):
            ch = kk[c:c + 64]
            mixed += bool((ch == 1).any() and (ch == 2).any() and (ch == 0).any())
    assert mixed >= 1
    # stage A: every centre of the list as a corner and as a contrast-thr non-corner
    for v in es.center_values(thr):
        at = placed[placed["centre"] == v]
        assert at["corner"].any(), v
        assert ((at["contrast"] == thr) & (at["length"] >= 9) & ~at["corner"]).any(), v
    lo, hi = placed[placed["corner"] & (placed["centre"] < thr)], placed[placed["corner"] & (placed["centre"] > 255 - thr)]
    assert len(lo) >= 16 and len(hi) >= 16                      # v - t wraps below 0, v + t leaves 8 bits


def _band_hits(img, thr):
    """{name: number of definition corners} on the places of a cell's band where stage A branches."""
    score = es.fast_corner_definition(img, thr)
    h, w = img.shape
    hit = dict.fromkeys(("first_col", "last_col", "first_row", "last_row", "odd_last_row", "wide_col31", "wide_col32"), 0)
    for (x0, y0, x1, y1) in es.bands_of_level(w, h):
        c = score[y0:y1, x0:x1] > 0
        bw, bh = x1 - x0, y1 - y0
        hit["first_col"] += c[:, 0].sum(); hit["last_col"] += c[:, -1].sum()
        hit["first_row"] += c[0].sum(); hit["last_row"] += c[-1].sum()
        if bh % 2 and bw <= 32:
            hit["odd_last_row"] += c[-1].sum()                  # two rows per step: the last step has one row inside
        if bw > 32:
            hit["wide_col31"] += c[:, 31].sum(); hit["wide_col32"] += c[:, 32].sum()
    return hit


def test_sheets_put_corners_on_every_edge_of_a_band(oracle_lib):
    total = {}
    for off in es.SHEET_OFFSETS:
        for k, v in _band_hits(es.sheet(20, off)[0], 20).items():
            total[k] = total.get(k, 0) + v
    for k in ("first_col", "last_col", "first_row", "last_row", "odd_last_row"):
        assert total[k] > 0, k
    w, h = es.NARROW_SIZE
    (bx0, by0, bx1, by1), = es.bands_of_level(w, h)
    assert bx1 - bx0 > 32 and (by1 - by0) % 2 == 1
    narrow = {}
    for off in es.NARROW_OFFSETS:
        img, placed = es.sheet(20, off, True)
        assert img.shape == (h, w) and placed["corner"].all() and len(placed) >= 12
        score = es.fast_corner_definition(img, 20)
        ys, xs = np.nonzero(score)
        assert _set(oracle_lib.fast9_16(img, 20, nms=False)) == sorted(zip(xs, ys, score[ys, xs]))
        for k, v in _band_hits(img, 20).items():
            narrow[k] = narrow.get(k, 0) + v
    assert narrow["wide_col31"] > 0 and narrow["wide_col32"] > 0 and narrow["first_col"] > 0 and narrow["last_col"] > 0


@pytest.mark.parametrize("thr,offset,narrow", [(20, es.SHEET_OFFSETS[1], False), (7, es.SHEET_OFFSETS[2], False), (20, es.NARROW_OFFSETS[1], True)])
def test_level_candidates_are_definition_then_nms_per_cell(oracle_lib, thr, offset, narrow):
    """cells_of_level + fast_corner_definition + nms_definition against the oracle's level-0 candidates, in order."""
    img, _ = es.sheet(thr, offset, narrow)
    ex = oracle_lib.OrbExtractorOracle(1000, 1.2, 8, thr, 7)
    ex.extract(img)
    c = ex.level_candidates(0)
    assert len(c) > 10
    assert es.level_candidates_definition(img, thr) == list(zip(c["x"].astype(int), c["y"].astype(int), c["response"].astype(int)))


def test_lattice_is_all_ties(oracle_lib):
    imgs = es.lattice_images()
    for name, (img, pts) in imgs.items():
        ex = oracle_lib.OrbExtractorOracle(es.LATTICE_FEATURES, 1.2, 8, 20, 7)
        ex.extract(img)
        c0 = ex.level_candidates(0)
        if name == "bars6":
            assert len(c0) == 0 and (es.fast_corner_definition(img, 20) == 254).sum() == 2 * len(pts)   # two equal neighbours: both vanish
            continue
        assert len(pts) > 700
        assert _set(c0, es.EDGE) == sorted((x, y, 254) for x, y in pts.tolist())       # every lattice point and nothing else
        assert es.level_candidates_definition(img, 20) == list(zip(c0["x"].astype(int), c0["y"].astype(int), c0["response"].astype(int)))
        quota = ex.tables()["per_level"]
        assert len(c0) > 3 * quota[0] and len(ex.level_keypoints(0)) == quota[0]
        if name != "lattice4":                                                         # period 6 -> 5: level 1 is one blob, repeated
            for l in (0, 1):
                c = ex.level_candidates(l)
                assert len(c) > 3 * quota[l]
                assert np.unique(c["response"], return_counts=True)[1].max() >= 0.9 * len(c), (name, l)


@functools.lru_cache(maxsize=None)
def marks_reference(oracle, frame=0):
    """The oracle's level-0 keypoints and descriptors of es.mark_frames()[frame]."""
    img, marks = es.mark_frames()[frame], es.oriented_marks()[1]
    ex = oracle.OrbExtractorOracle(1000, 1.2, 8, 20, 7)
    kps, desc = ex.extract(img)
    n0 = len(ex.level_keypoints(0))
    return img, marks, ex.tables()["max_x"], kps[:n0], desc[:n0], ex.level_blurred(0)


def test_oriented_marks_reach_every_branch_of_the_angle(oracle_lib):
    img, marks, max_x, k0, _, _ = marks_reference(oracle_lib)
    assert (k0["octave"] == 0).all()
    n = dict.fromkeys(("E", "W", "S", "N", "++", "+-", "-+", "--", "O"), 0)
    err, m10_max, m01_max = 0.0, 0, 0
    for kp in k0:
        m10, m01 = es.moments(img, int(kp["x"]), int(kp["y"]), max_x)
        a = np.float32(oracle_lib.fast_atan2(m01, m10))
        assert a.view(np.uint32) == kp["angle"].view(np.uint32)
        t = math.degrees(math.atan2(m01, m10)) % 360
        err = max(err, min(abs(float(a) - t), 360 - abs(float(a) - t)))
        m10_max, m01_max = max(m10_max, abs(m10)), max(m01_max, abs(m01))
        if m01 == 0 and m10 == 0: n["O"] += 1
        elif m01 == 0: n["E" if m10 > 0 else "W"] += 1
        elif m10 == 0: n["S" if m01 > 0 else "N"] += 1
        elif abs(m10) == abs(m01): n[("+" if m10 > 0 else "-") + ("+" if m01 > 0 else "-")] += 1
    assert err < 0.3
    assert all(n[k] >= 4 for k in "EWSN") and all(n[k] >= 2 for k in ("++", "+-", "-+", "--")) and n["O"] >= 1, n
    # the half-plane marks: every pixel of one side of the patch at 255, the other side at 0
    rows = [15] + [int(max_x[v]) for v in range(1, 16)]
    assert m10_max == 255 * sum((1 if v == 0 else 2) * sum(range(1, d + 1)) for v, d in enumerate(rows))
    assert m01_max == 255 * sum(v * (2 * d + 1) for v, d in enumerate(rows))


@pytest.mark.parametrize("frame", [0, 1, 2])
def test_angle_zero_descriptors_are_tied_tests(oracle_lib, frame):
    """The marks, and their mirror images left-right and top-bottom (the GPU test runs the three as one batch)."""
    img, _, _, k0, d0, blurred = marks_reference(oracle_lib, frame)
    assert np.array_equal(blurred, es.blur_definition(img))
    zero = np.nonzero(k0["angle"].view(np.uint32) == 0)[0]
    assert len(zero) >= 8
    for i in zero:
        desc, ties = es.brief_at_angle_zero(blurred, int(k0["x"][i]), int(k0["y"][i]))
        assert np.array_equal(desc, d0[i])
        assert ties >= 128                                       # at least half of the 256 bits are 0 because t0 == t1


def test_saturated_images_blur(oracle_lib):
    imgs = es.saturated_images()
    assert set(imgs) == {"white_with_patch", "checker1", "checker2", "stripes7", "noise"}
    for name, img in imgs.items():
        assert img.shape == (120, 160) and img.min() == 0 and img.max() == 255, name
        assert np.array_equal(oracle_lib.gaussian_blur_7x7_s2(img), es.blur_definition(img)), name
    assert (imgs["white_with_patch"] == 255).mean() > 0.8
    # the 16-bit horizontal sum reaches its largest value, 256 * 255, and the result 255
    assert es.blur_definition(imgs["white_with_patch"]).max() == 255
    ex = oracle_lib.OrbExtractorOracle(500, 1.2, 8, 20, 7)
    for name in ("white_with_patch", "noise"):
        ex.extract(imgs[name])
        assert np.array_equal(ex.level_blurred(0), es.blur_definition(imgs[name])), name


def test_mutations_fail_the_asserts_above(oracle_lib):
    """Three wrong implementations, each in a copy of the definition; for each, the comparison that an assert of this file makes
    holds for the right definition (asserted above) and does not hold for the wrong one."""
    # 1. stage B without its second network: a pixel whose compass test passes both ways gets the darker arcs only
    img, _ = es.sheet(20, es.SHEET_OFFSETS[1])
    ex = oracle_lib.OrbExtractorOracle(1000, 1.2, 8, 20, 7)
    ex.extract(img)
    c = ex.level_candidates(0)
    want = list(zip(c["x"].astype(int), c["y"].astype(int), c["response"].astype(int)))
    cd, cb = es.compass_flags(img, 20)
    both = cd & cb
    full, dark_only = es.fast_corner_definition(img, 20), es.fast_corner_definition(img, 20, networks=("darker",))
    h, w = img.shape

    def candidates(score):
        out = []
        for (bx0, by0, bx1, by1) in es.bands_of_level(w, h):
            out += [(bx0 + x - es.EDGE, by0 + y - es.EDGE, s) for (x, y, s) in es.nms_definition(score[by0:by1, bx0:bx1])]
        return out
    assert candidates(full) == want
    assert candidates(np.where(both, dark_only, full)) != want
    # 2. NMS with >= : the two equal neighbours of a bar both survive
    bars, pts = es.lattice_images()["bars6"]
    assert es.level_candidates_definition(bars, 20) == []
    assert len(es.level_candidates_definition(bars, 20, op=np.greater_equal)) == 2 * len(pts)
    # 3. descriptor with <= : every tied test gives a 1
    _, _, _, k0, d0, blurred = marks_reference(oracle_lib)
    i = int(np.nonzero(k0["angle"].view(np.uint32) == 0)[0][0])
    x, y = int(k0["x"][i]), int(k0["y"][i])
    assert np.array_equal(es.brief_at_angle_zero(blurred, x, y)[0], d0[i])
    assert not np.array_equal(es.brief_at_angle_zero(blurred, x, y, op=np.less_equal)[0], d0[i])
