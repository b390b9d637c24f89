"""One-off differential sweep on the GPU box: random image sizes / extractor configurations / matcher inputs / BA and pose problems,
product vs oracle.  Not part of the test suite (the suite pins fixed cases); run it after kernel changes:  python tools/fuzz_parity.py 120
Arguments: seconds [seed [stereo batch [stereo slice]]].  A stereo batch of 8 or more members (default 10) walks frames of more than 1024
keypoints in slices; a stereo slice > 0 is set as YDORB_STEREO_SLICE (read per call), 0 (default) draws one per case: none, 1 for small
frames, or a random length."""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import ydorbslam_amd as y
from oracle import orb_oracle as oo
from ydorbslam_amd.synth import synth_frame, synth_ba_problem, synth_pose_problem, synth_vocabulary
from helpers import bow_nodes, feature_vector, projection_queries

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 12345)
stereo_batch = max(1, int(sys.argv[3])) if len(sys.argv) > 3 else 10
stereo_slice = int(sys.argv[4]) if len(sys.argv) > 4 else 0
t0 = time.time()
n_ex = n_ma = n_ba = n_po = n_st = n_bw = 0
while time.time() - t0 < budget:
    # ---- extractor
    w, h = int(rng.integers(60, 1400)), int(rng.integers(60, 800))
    nf = int(rng.choice([100, 500, 1000, 2000, 4000])); sf = float(rng.choice([1.1, 1.2, 1.5, 2.0, 2.3])); nl = int(rng.integers(1, 9))
    thr = int(rng.choice([7, 12, 20, 40]))
    img = synth_frame(w, h, int(rng.integers(0, 1000)))
    mode = rng.integers(0, 4)
    if mode == 1: img[: h // 2] = 100
    if mode == 2: img = (img // 4 + 90).astype(np.uint8)          # low contrast: sparse, deep quad-trees
    try:
        g = y.OrbExtractor(nf, sf, nl, thr, 7); c = oo.OrbExtractorOracle(nf, sf, nl, thr, 7)
    except Exception as e:  # unsupported configuration on either side must be an error on both
        print("config rejected:", (w, h, nf, sf, nl, thr), str(e)[:80]); continue
    try:
        gk, gd = g.extract(img)
    except y.YdorbError as e:
        print("extract rejected:", (w, h, nf, sf, nl, thr), str(e)[:100]); continue
    ck, cd = c.extract(img)
    assert gk.tobytes() == ck.tobytes() and np.array_equal(gd, cd), ("extractor", w, h, nf, sf, nl, thr, mode)
    n_ex += 1
    # ---- matcher on this frame vs a shifted copy
    if len(gk) > 50 and w > 200 and h > 200:
        img2 = np.roll(img, (int(rng.integers(-6, 7)), int(rng.integers(-6, 7))), (0, 1))
        kb, db = c.extract(img2)
        if len(kb) > 20:
            tab = c.tables()["scale"]
            for m_ in (0, 1, 2, 7):
                q = projection_queries(ck, tab, 0, 0, float(rng.choice([3, 7, 15])), m_ if m_ < 3 else 1, seed=int(rng.integers(0, 1 << 30)), stereo=False)
                if m_ == 7:
                    q["min_level"], q["max_level"] = -1, -1
                taken0 = (rng.random(len(kb)) < 0.1).astype(np.uint8); a0 = np.where(taken0 > 0, 100000 + np.arange(len(kb)), -1).astype(np.int32)
                fo = oo.FrameOracle(kb, db, (0.0, float(w), 0.0, float(h)), None)
                r = fo.search_by_projection(m_, q, cd, 0.8, True, taken0, a0, orb_dist=64)
                mm = y.OrbMatcher(0.8, True)
                p = mm.search_by_projection(m_, y.FrameView(kb, db, (0.0, float(w), 0.0, float(h)), None), q, cd, taken0, a0, orb_dist=64)
                assert p[0] == r[0] and np.array_equal(p[1], r[1]) and np.array_equal(p[2], r[2]), ("projection", m_, w, h)
            fa, fb = feature_vector(bow_nodes(cd, 4)), feature_vector(bow_nodes(db, 4))
            va = (rng.random(len(ck)) > 0.2).astype(np.uint8); vb = (rng.random(len(kb)) > 0.2).astype(np.uint8)
            for m_ in (3, 4):
                r = oo.search_by_bow(m_, ck, cd, va, fa, kb, db, vb, fb, 0.75, True)
                p = y.OrbMatcher(0.75, True).search_by_bow(m_, ck, cd, va, y.FeatureVector(*fa), kb, db, vb if m_ == 4 else None, y.FeatureVector(*fb))
                assert p[0] == r[0] and np.array_equal(p[1], r[1]), ("bow", m_)
            n_ma += 1
    # ---- stereo association on this frame vs a copy moved left by a random disparity (second handle = the right extractor)
    if len(gk) > 30 and w > 120 and rng.random() < 0.5:
        dsp = int(rng.integers(0, 40))
        right = np.clip(np.roll(img, -dsp, 1).astype(np.int16) + rng.integers(-3, 4, img.shape), 0, 255).astype(np.uint8)
        g2 = y.OrbExtractor(nf, sf, nl, thr, 7); c2 = oo.OrbExtractorOracle(nf, sf, nl, thr, 7)
        rk, rd = g2.extract(right); ork, ord_ = c2.extract(right)
        c.extract(img)   # the matcher section left the shifted copy's pyramid in the left oracle
        assert rk.tobytes() == ork.tobytes()
        if 0 < len(rk) <= 8192:
            lk = gk.copy()
            if rng.random() < 0.3 and len(lk) > 5:   # rows outside the table / negative x
                lk["y"][int(rng.integers(0, len(lk)))] = float(h) + 0.5
                lk["x"][int(rng.integers(0, len(lk)))] = -1.0
            lv_l = [c.level_padded(l)[19:19 + c.level_dims(l)[1], 19:19 + c.level_dims(l)[0]] for l in range(nl)]
            lv_r = [c2.level_padded(l)[19:19 + c2.level_dims(l)[1], 19:19 + c2.level_dims(l)[0]] for l in range(nl)]
            tb = c.tables(); bf = float(rng.choice([20.0, 40.0, 386.0])); bl = float(rng.choice([0.05, 0.1, 0.54]))
            if rng.random() < 0.3:   # descriptor-dependent index chains
                gd = gd.copy(); gd[1::2] = rng.integers(0, 256, gd[1::2].shape, dtype=np.uint8)
            for by_kp in (False, True):
                o_ = oo.stereo_matches(lk, gd, rk, rd, lv_l, lv_r, tb["scale"], tb["inv_scale"], bf, bl, by_kp)
                p_ = y.OrbMatcher().stereo_matches(g, g2, lk[None], gd[None], [len(lk)], rk[None], rd[None], [len(rk)], bf, bl, by_kp)
                if not (p_[2][0] == o_[2] and p_[3][0] == o_[3] and p_[0][0].tobytes() == o_[0].tobytes() and p_[1][0].tobytes() == o_[1].tobytes()):
                    bad = np.flatnonzero((p_[0][0].view(np.uint32) != o_[0].view(np.uint32)) | (p_[1][0].view(np.uint32) != o_[1].view(np.uint32)))
                    print("stereo mismatch: kept", p_[2][0], o_[2], "status", p_[3][0], o_[3], "n", len(lk), len(rk), "bad slots", bad[:10], len(bad))
                    for i in bad[:5]:
                        print("  slot", i, "gpu", p_[0][0][i], p_[1][0][i], "oracle", o_[0][i], o_[1][i], "kp", lk[i])
                    raise AssertionError(("stereo", w, h, nf, sf, nl, thr, dsp, by_kp, bf, bl))
            # the sliced replay: a batch over this one pyramid pair (frame step 0), members cut to ragged lengths around the slice edges
            if stereo_batch > 1 or stereo_slice > 0:
                n_ = len(lk)
                sl_ = stereo_slice if stereo_slice > 0 else int(rng.choice([0, 1 if n_ <= 400 else 0, int(rng.integers(2, max(n_, 3)))]))
                edge = sl_ if sl_ > 0 else 1024
                cuts = [n_, min(n_, edge), min(n_, edge + 1), max(0, min(n_, edge) - 1), 0] + [int(x) for x in rng.integers(0, n_ + 1, max(stereo_batch - 5, 0))]
                cuts = cuts[:stereo_batch]
                if sl_ > 0: os.environ["YDORB_STEREO_SLICE"] = str(sl_)
                try:
                    B_ = len(cuts)
                    p_ = y.OrbMatcher().stereo_matches(g, g2, np.tile(lk, (B_, 1)), np.tile(gd, (B_, 1, 1)), cuts, np.tile(rk, (B_, 1)), np.tile(rd, (B_, 1, 1)),
                                                       [len(rk)] * B_, bf, bl, False, left_frames=(0, 0), right_frames=(0, 0))
                finally:
                    os.environ.pop("YDORB_STEREO_SLICE", None)
                for i_, c_ in enumerate(cuts):
                    o_ = oo.stereo_matches(lk[:c_], gd[:c_], rk, rd, lv_l, lv_r, tb["scale"], tb["inv_scale"], bf, bl, False)
                    ok_ = (p_[2][i_] == o_[2] and p_[3][i_] == o_[3] and p_[0][i_, :c_].tobytes() == o_[0].tobytes() and p_[1][i_, :c_].tobytes() == o_[1].tobytes()
                           and np.all(p_[1][i_, c_:] == -1))
                    assert ok_, ("stereo batch", w, h, nf, sf, nl, thr, dsp, bf, bl, "slice", sl_, "member", i_, "nL", c_, "of", n_)
            n_st += 1
    # ---- vocabulary transform + distinctive descriptors on this frame's descriptors
    if len(gk) > 0 and len(gk) <= 8192 and rng.random() < 0.4:
        wgt, nrm = int(rng.integers(0, 4)), int(rng.integers(0, 3))
        tree = synth_vocabulary(int(rng.integers(2, 11)), int(rng.integers(1, 6)), seed=int(rng.integers(0, 1 << 30)),
                                early_leaf_frac=float(rng.choice([0.0, 0.2, 0.5])), stopped_frac=float(rng.choice([0.0, 0.1, 0.5])))
        leaves = np.flatnonzero(np.diff(tree["child_begin"]) == 0)
        dd = np.where(rng.random((len(gd), 1)) < 0.5, gd, tree["node_desc"][rng.choice(leaves, len(gd))])   # half of them close to words
        lup = int(rng.integers(0, 7))
        voc = y.Vocabulary(tree, ["TF_IDF", "TF", "IDF", "BINARY"][wgt], ["none", "L1", "L2"][nrm])
        got = voc.transform([dd, dd[: len(dd) // 3]], lup)
        for d_, g_ in zip([dd, dd[: len(dd) // 3]], got):
            o_ = oo.bow_transform(tree, d_, lup, wgt, nrm)
            assert all(np.array_equal(np.asarray(a_).view(np.uint8) if hasattr(a_, "view") else a_, np.asarray(b_).view(np.uint8) if hasattr(b_, "view") else b_)
                       for a_, b_ in zip(g_, o_)), ("bow", wgt, nrm, lup)
        groups = [gd[int(a_):int(a_) + int(m_)] for a_, m_ in zip(rng.integers(0, max(len(gd) - 70, 1), 40), rng.integers(0, 70, 40))]
        bi = y.OrbMatcher().distinctive_descriptors(groups)
        assert list(bi) == [oo.distinctive_descriptor(g_) if len(g_) else -1 for g_ in groups], "distinctive"
        n_bw += 1
    # ---- BA + pose
    if rng.random() < 0.3:
        n_obs, mono = int(rng.integers(2, 8)), float(rng.choice([0, 0.3, 1.0]))
        prob = synth_ba_problem(int(rng.integers(3, 40)), int(rng.integers(30, 1500)), n_obs, seed=int(rng.integers(0, 1 << 30)),
                                outlier_frac=float(rng.choice([0, 0.05, 0.2])), mono_frac=mono, n_fixed=int(rng.integers(1, 3)))
        r = oo.ba_solve(prob); p = y.Optimizer.local_bundle_adjust(prob)
        # Two monocular observations per point leave the problem barely constrained: chi2 falls to ~1e-25 and the accept / reject
        # sequence of the LM trials depends on the last bits of the sums (3 of 6383 such problems differed from the oracle's sequence
        # in tools/fuzz_ba.py, with the pre-MFMA Cholesky as well); there only the outlier list and the float poses are compared.
        if not (n_obs == 2 and mono == 1.0):
            assert len(p["log"]) == len(r["log"]) and np.allclose(p["log"][:, 0], r["log"][:, 0], rtol=1e-6), "ba chi2"
        assert np.array_equal(p["outlier"], r["outlier"]), "ba"
        assert np.allclose(p["poses"].astype(np.float32), r["poses"].astype(np.float32), rtol=1e-4, atol=1e-6), "ba poses"
        n_ba += 1
        pp = [synth_pose_problem(int(rng.integers(3, 1500)), seed=int(rng.integers(0, 1 << 30)), outlier_frac=float(rng.choice([0, 0.1, 0.4])),
                                 mono_frac=float(rng.choice([0, 0.5, 1.0]))) for _ in range(5)]
        for p_, g_ in zip(pp, y.Optimizer.optimize_poses(pp)):
            r_ = oo.pose_optimize(p_)
            assert g_["inliers"] == r_["inliers"] and np.array_equal(g_["outlier"], r_["outlier"]), ("pose", len(p_["info"]))
            n_po += 1
print("fuzz ok: %d extractor configs, %d matcher scenes, %d stereo pairs, %d vocabulary / distinctive-descriptor cases, %d BA problems, %d pose problems in %.0f s" % (n_ex, n_ma, n_st, n_bw, n_ba, n_po, time.time() - t0))
