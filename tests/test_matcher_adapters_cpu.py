"""CPU half of the executed matcher / stereo adapters (tests/cpp_host/matcher_adapters_run.cpp, tests/matcher_adapters_support.py): the
host program compiles and links, each independent statement is held to a plain float64 evaluation of the same float32 inputs, each
scenario shows every branch its GPU test relies on (on the statement and the serial oracle alone), and each scenario tells the
documented quirks from their alternative readings.  Run with -s to see the figures."""
import numpy as np
import pytest

import matcher_adapters_support as S

SIM_SCALES = (0.8, 1.0, 1.3)


def test_program_builds_and_links(tmp_path):
    """matcher_adapters_run.cpp instantiates the eight adapter bodies against stand-ins with real storage and links against libydorb.so."""
    import os
    import ydorbslam_amd as y
    if not os.path.exists(y.library_path()):
        y.build_library()
    assert os.path.exists(S.build_program(str(tmp_path)))


def _rows(name, sc):
    """(label, live mask, float32 rows, float64 rows) of one scenario's statement."""
    if name == "mappoint":
        st = S.statement_mappoint(sc)
        q = st["q"]
        return [(name, st["live"], dict(u=q["u"], v=q["v"], ur=q["ur"], r=q["r"], level=q["level"], ok=st["live"]), S.double_mappoint(sc))]
    if name == "reloc":
        st = S.statement_reloc(sc)
        return [(name, st["live"], st["g"], S.double_reloc(sc))]
    if name in ("sim", "fusesim"):
        st = S.statement_sim(sc)
        return [("%s scale %.1f" % (name, sc.args["scale"]), st["live"], st["g"], S.double_sim(sc))]
    if name == "fuse":
        st = S.statement_fuse(sc)
        return [(name, st["live"], st["g"], S.double_fuse(sc))]
    (a, b), _, _ = S.statement_sim3(sc)
    da, db = S.double_sim3(sc)
    return [("sim3 1->2", a["live"], a["g"], da), ("sim3 2->1", b["live"], b["g"], db)]


def _scenarios():
    out = [("mappoint", S.scenario_mappoint()), ("reloc", S.scenario_reloc()), ("fuse", S.scenario_fuse()), ("sim3", S.scenario_sim3())]
    out += [("sim", S.scenario_sim(s)) for s in SIM_SCALES] + [("fusesim", S.scenario_fusesim(s)) for s in SIM_SCALES]
    return out


def test_statements_against_float64():
    """Every statement's rows against a double evaluation of the same float inputs.  Tolerance, from the formats alone (eps = 2^-24,
    the relative error of one rounding to float), as in tests/test_frustum_cpu.py::test_noise_free_scene_against_numpy: each component of
    Pc = R P + t carries a rounding per product and per sum, relative to |R row| |P| + |t| <= 2 sqrt(3) |P|max + |t|max (the factor 2
    covers the three products and three sums against terms that size), so x / z is off by at most 2 eps (2 sqrt(3) |P| + |t|) / z
    (1 + |x / z|), and u = fx * x / z + cx adds a multiply, a divide and an add on terms no larger than |u| + cx, with the error of u
    itself that is 4 eps (|u| + cx): |du| <= fx * 2 eps (2 sqrt(3) |P| + |t|) (1 + |x/z|) / z + 4 eps (|u| + cx); v alike.  The Sim3
    forms use R = sR / scale, whose entries carry the rounding of scale and of the quotient: 2 eps more per entry, i.e. 2 sqrt(3) |P| more
    inside the bracket.  ur = u - bf / z adds a divide and a subtract: 4 eps (|u| + bf / z) more.  r = th * scaleFactor[level] is one
    rounded product of the same two floats: eps r (mappoint: thd * factor * scaleFactor, two roundings, 2 eps r; its u, v, ur are copied,
    bound 0).  These bounds are loose by about a factor of ten for u and v (the printed fractions): they are worst cases of every
    rounding at once.
    flags and level: an entry whose float and double decisions differ - the predicates, or the predicted level, which every live entry
    has whether it is searched or not - sits on a boundary to within those errors and is left out of the comparison of u, v, ur, r.
    The OPERATIVE assertion for flags and level is therefore the cap on those entries, at most 1 % of a scenario's live entries (the
    seeds are chosen so; every scenario reads 0): with a wrong predicate or level rule in the statement the share would be far above
    it.  r is compared on every live entry off the boundary, rejected ones included, since the adapters fill it for them too."""
    for name, sc in _scenarios():
        for label, live, g, d in _rows(name, sc):
            live = np.asarray(live, bool)
            n = int(live.sum())
            assert n > 100, label
            boundary = live & ((np.asarray(g["ok"], bool) != d["ok"]) | (g["level"] != d["level"]))
            share = boundary.sum() / n
            both = live & np.asarray(g["ok"], bool) & d["ok"] & ~boundary
            worst = {}
            for k in ("u", "v", "ur", "r"):
                if k not in d or k not in g:
                    continue
                rows = (live & ~boundary) if k == "r" else both
                gap = np.abs(np.asarray(g[k], np.float64) - d[k])[rows]
                tol = d["tol"][k][rows]
                assert np.all(gap <= tol), (label, k, gap.max())
                worst[k] = float((gap / np.maximum(tol, 1e-300)).max()) if np.any(tol > 0) else 0.0
            print("%-18s entries %3d, searched %3d, boundary share %.4f, largest gap / format bound: %s" %
                  (label, n, int(both.sum()), share, ", ".join("%s %.2f" % kv for kv in worst.items())))
            assert share <= 0.01, (label, share)
            assert both.sum() >= 30, label
    sc = S.scenario_tri()
    ex, ey = S.statement_tri(sc)["epipole"]
    dx, dy = S.double_tri(sc)
    # C2 = R2 Cw + t2 with |Cw|, |t2| < 1: each component within 8 eps; divided by |C2z| and times fx, plus 4 eps (|e| + cx): a worst
    # case some hundred times the gap seen, still three orders below the pixels by which the alternative readings move the epipole
    k2 = sc.kfs[1]
    C2z = abs(float((S.gemv32(k2["R"], sc.kfs[0]["O"][None])[0] + k2["t"])[2]))
    tol = 500.0 * 16 * S.EPS / C2z * (1 + abs(dx - 319.5) / 500.0) + 4 * S.EPS * (abs(dx) + 319.5)
    print("tri epipole (%.3f, %.3f), gap (%.2e, %.2e), bound %.2e" % (ex, ey, abs(ex - dx), abs(ey - dy), tol))
    assert abs(float(ex) - dx) <= tol and abs(float(ey) - dy) <= tol and 0 < ex < S.W and 0 < ey < S.H


def test_scenarios_are_non_trivial():
    """On the statement and the serial oracle alone: every branch the GPU tests name occurs at least 3 times and at least 10 matches
    are accepted, per adapter and per parameter the GPU tests run."""
    o = S.OracleSearch()
    cases = [("mappoint", S.scenario_mappoint(), "mappoint")]
    cases += [("reloc", S.scenario_reloc(orb_dist=d, check_ori=c), "reloc" if c else "reloc_no_ori") for d in (100, 40) for c in (True, False)]
    cases += [("sim", S.scenario_sim(s), "sim") for s in SIM_SCALES] + [("fusesim", S.scenario_fusesim(s), "fusesim") for s in SIM_SCALES]
    cases += [("fuse", S.scenario_fuse(), "fuse"), ("sim3", S.scenario_sim3(), "sim3")]
    cases += [("tri", S.scenario_tri(stereo_only=s, check_ori=c), "tri_stereo_only" if s else "tri") for s in (False, True) for c in (False, True)]
    seen = {}
    for name, sc, req in cases:
        n, vec, state, counts = S.CASES[name][1](sc, o)
        print(name, {k: v for k, v in sc.args.items() if k in ("orb_dist", "check_ori", "scale", "stereo_only")}, "returns", n, counts)
        S.check_counts(req, counts)
        assert max(len(k["kps"]) for k in sc.kfs) <= 400 and len(sc.frame["kps"]) <= 400 and sc.n <= 300
        seen.setdefault(name, []).append((sc.args, counts, vec))
    by = {(a["orb_dist"], a["check_ori"]): c for a, c, _ in seen["reloc"]}
    assert by[(100, False)]["matches"] >= by[(40, False)]["matches"] + 10            # the two orbDist values accept different sets
    assert by[(100, True)]["culled"] >= 1 and by[(100, False)]["culled"] == 0
    tri = {(a["stereo_only"], a["check_ori"]): (c, v) for a, c, v in seen["tri"]}
    assert tri[(False, False)][0]["matches"] > tri[(True, False)][0]["matches"] >= 10
    assert tri[(False, False)][0]["matches"] > tri[(False, True)][0]["matches"]       # the orientation check removes pairs
    assert tri[(False, False)][0]["mono_pairs"] >= 3 and tri[(True, False)][0]["mono_pairs"] == 0
    for (stereo_only, _), (c, _) in tri.items():       # the epipole alone removes the 24 mono twins round it; stereo pairs are exempt
        assert c["removed_by_epipole"] == c["changed_by_epipole"] == (0 if stereo_only else 24)
    for _, v in tri.values():
        assert np.all(np.diff(v[0::2]) > 0)                                          # pairs in first-index order


def _changed(a, b):
    return int(((a["level"] != b["level"]) | (a["flags"] != b["flags"]) | (a["r"] != b["r"]) | (a["min_level"] != b["min_level"]) |
                (a["max_level"] != b["max_level"])).sum())


def test_reloc_scenario_tells_the_camera_centre_readings_apart():
    """searchByProjectionInKeyFrameAndCurrentFrame measures the distance to -R t, as the reference writes it (SURVEY.md:291), not to the
    camera centre -R^T t.  With a rotation of 20 degrees and a translation of a metre the two differ by decimetres: the statement with
    the other reading must change the level, flags or radius of at least 10 queries."""
    sc = S.scenario_reloc()
    n = _changed(S.statement_reloc(sc, "R")["q"], S.statement_reloc(sc, "Rt")["q"])
    print("reloc: -R t against -R^T t changes %d of %d queries" % (n, len(sc.kfs[0]["kps"])))
    assert n >= 10


@pytest.mark.parametrize("name", ["sim", "fusesim"])
def test_sim_scenarios_tell_the_translation_readings_apart(name):
    """SimProjection takes t = S[:3, 3] undivided, citing the reference's :241-247; ORB-SLAM2 divides the translation by the scale at this
    place.  This suite PINS THE HEADER'S READING (DESIGN.md section 6 says so); parity with the reference's binary stays unpinned, so a
    maintainer who holds the reference knows to look.  At scales 0.8 and 1.3 the alternative t / scale must change at least 10 queries;
    at scale 1.0 the two readings are the same numbers and nothing may change."""
    for scale in SIM_SCALES:
        sc = (S.scenario_sim if name == "sim" else S.scenario_fusesim)(scale)
        n = _changed(S.statement_sim(sc)["q"], S.statement_sim(sc, t_over_scale=True)["q"])
        print("%s scale %.1f: t against t / scale changes %d of %d queries" % (name, scale, n, len(sc.args["list"])))
        assert (n == 0) if scale == 1.0 else (n >= 10)


@pytest.mark.parametrize("check_ori", [False, True])
def test_tri_scenario_tells_the_epipole_readings_apart(check_ori):
    """searchForTriangulation takes the epipole as the FIRST keyframe's stored centre (-R1^T t1) seen by the SECOND.  With the centre
    read as -R1 t1, or with the second keyframe's centre projected into the first, the epipole lands some 140 and 85 px away: the mono
    twins round the true one pair up, and the serial oracle's pairs must differ in at least 10 places under each reading."""
    sc = S.scenario_tri(stereo_only=False, check_ori=check_ori)
    o = S.OracleSearch()
    e0 = S.statement_tri(sc)["epipole"]
    _, base = S.tri_pairs(sc, o, e0)
    for reading in ("Rt", "swap"):
        e = S.statement_tri(sc, reading)["epipole"]
        _, alt = S.tri_pairs(sc, o, e)
        print("tri check_ori %s: epipole (%.1f, %.1f), reading %s (%.1f, %.1f) changes %d of %d pairs" %
              (check_ori, e0[0], e0[1], reading, e[0], e[1], int((alt != base).sum()), int((base >= 0).sum())))
        assert (alt != base).sum() >= 10


def test_mappoint_scenario_tells_the_level_window_and_the_radii_apart():
    """Level window level-1 .. level against level-1 .. level+1, and the radii 2.5 (viewCos > 0.998) / 4.0 against their swap: each
    alternative changes at least 10 queries, and the serial oracle's matches change with each (the twins sit at the predicted level,
    which the +1 window's lower bound drops, and just outside the radius as written)."""
    sc = S.scenario_mappoint()
    base = S.statement_mappoint(sc)
    o = S.OracleSearch()
    n0, ref, _, counts = S.expected_mappoint(sc, o)
    for label, alt in (("max level + 1", S.statement_mappoint(sc, max_level_plus=1)), ("radii swapped", S.statement_mappoint(sc, swap_radii=True))):
        n = _changed(base["q"], alt["q"])
        _, assigned = o.projection(0, sc.frame, alt["q"], alt["qd"], alt["taken"], np.full(len(sc.frame["kps"]), -1, np.int32), ratio=float(sc.args["ratio"]))
        got = sc.frame["mp_of"].copy()
        got[assigned >= 0] = sc.args["list"][assigned[assigned >= 0]]
        print("mappoint: %s changes %d of %d queries and %d frame slots" % (label, n, len(base["q"]), int((got != ref).sum())))
        assert n >= 10 and (got != ref).sum() >= 10
    assert counts["radius_2_5"] >= 3 and counts["radius_4_0"] >= 3


def test_stereo_scenario_keeps_enough_matches(oracle_lib):
    """The synthetic pair of the stereo GPU test, on the CPU oracle alone: at least 30 matches with either indexing."""
    for by_kp in (False, True):
        r = S.stereo_oracle(oracle_lib, by_kp)
        print("stereo %dx%d, %d features, by keypoint %s: left %d, right %d, kept %d, status %d" %
              (S.STEREO_W, S.STEREO_H, S.STEREO_NF, by_kp, len(r["kl"]), len(r["kr"]), r["kept"], r["status"]))
        assert r["kept"] >= 30 and (r["rx"] >= 0).sum() == r["kept"]
