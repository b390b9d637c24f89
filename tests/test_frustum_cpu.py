"""Tracking::searchLocalPoints' geometry without a GPU: the CPU restatement (tests/frustum_ref) on hand-built rows and against numpy,
the level threshold table against the formula, the adapter's syntax check and the ABI's argument checks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import frustum_support as S
from frustum_support import ROOT, f32


def _hand():
    views, logs, table, lists, skips, names = S.hand_batch()
    return names, S.ref_cull(views, logs, table, lists, skips)


@pytest.mark.parametrize("name", sorted(S.hand_rows()))
def test_hand_built_row_gives_its_exit_code(name):
    names, res = _hand()
    want, r = S.hand_rows()[name], res[names.index(name)]
    assert r["status"][0] == want["status"], (name, r["status"][0])
    assert r["n_in_view"] == int(want["status"] == 0)
    row = r["rows"][0]
    if want["status"] != 0:
        assert row.tobytes() == bytes(20)                      # rows of entries not in view are all zero
        return
    if want["level"] is not None:
        assert row["level"] == want["level"]
    for k in ("u", "v", "ur", "view_cos"):
        assert bool(np.isnan(row[k])) == (k in want["nan"]), k


def test_hand_built_rows_cover_every_exit_and_both_clamps():
    rows = S.hand_rows()
    assert {r["status"] for r in rows.values()} == set(range(7))
    assert rows["clamp_low"]["level"] == 0 and rows["clamp_high"]["level"] == 7
    assert {"pcz_zero_inf", "pcz_zero_nan", "nan_position", "dist_zero"} <= set(rows)


def test_in_view_row_values():
    """The plain in-view row against the formulas in double: P = (0.2, 0.1, 4) seen from the origin."""
    names, res = _hand()
    row = res[names.index("in_view")]["rows"][0]
    assert abs(row["u"] - (S.K[0] * 0.2 / 4 + S.K[2])) < 1e-3 and abs(row["v"] - (S.K[1] * 0.1 / 4 + S.K[3])) < 1e-3
    assert abs(row["ur"] - (row["u"] - S.BF / 4)) < 1e-3 and abs(row["view_cos"] - 1) < 1e-6


def _numpy_rows(view, table, idx):
    """isInCameraFrustum's quantities from the same float inputs in double."""
    f64 = lambda a: np.asarray(a, f32).astype(np.float64)
    R, t, Ow = f64(view.Rcw[:]).reshape(3, 3), f64(view.tcw[:]), f64(view.Ow[:])
    P, Pn = f64(table.pos_min[idx, :3]), f64(table.normal_max[idx, :3])
    Pc = P @ R.T + t
    u = f64(view.fx) * Pc[:, 0] / Pc[:, 2] + f64(view.cx)
    v = f64(view.fy) * Pc[:, 1] / Pc[:, 2] + f64(view.cy)
    PO = P - Ow
    dist = np.linalg.norm(PO, axis=1)
    return dict(u=u, v=v, ur=u - f64(view.bf) / Pc[:, 2], view_cos=(PO * Pn).sum(axis=1) / dist, z=Pc[:, 2], P=P, dist=dist)


def test_noise_free_scene_against_numpy():
    """The restatement's in-view rows against a double evaluation of the same float inputs.  Tolerance, from the formats alone (eps =
    2^-24, the relative error of one rounding to float): Pc carries one rounding each, relative to |R row| |P| + |t| <= 2 |P| + |t|, so
    PcX / PcZ is off by at most 2 eps (2 |P| + |t|) / PcZ (1 + |PcX| / PcZ), and u = fx * PcX * invz + cx adds four roundings of terms no
    larger than |u| + cx: |du| <= fx * 2 eps * (2 |P| + |t|) * (1 + |x/z|) / z + 4 eps (|u| + cx).  ur adds bf * invz (two roundings and
    invz's own) and one subtraction: 4 eps more of (|u| + bf / z).  viewCos is one rounding of a double quotient whose denominator
    carries dist's rounding and whose PO carries three (relative to |P| + |Ow|): |dcos| <= eps (2 + 2 (|P| + |Ow|) / dist).  The
    measured gaps are printed (DESIGN.md section 6g records them); the level must agree wherever the double ratio is further than
    4 eps (relative) from a threshold."""
    views, logs, table, lists, skips = S.scene()
    eps = 2.0 ** -24
    worst = dict(u=0.0, v=0.0, ur=0.0, view_cos=0.0)
    checked = 0
    for f in (0, 2):
        idx = np.asarray(lists[f])
        r = S.ref_cull([views[f]], [logs[f]], table, [idx], [np.zeros(len(idx), np.uint8)])[0]
        ok = r["status"] == 0
        assert ok.sum() > 20
        w = _numpy_rows(views[f], table, idx)
        t = np.abs(np.asarray(views[f].tcw[:], np.float64)).max()
        Pm, Om = np.abs(w["P"]).max(axis=1), np.abs(np.asarray(views[f].Ow[:], np.float64)).max()
        z = w["z"]
        geo = 2 * eps * (2 * 1.7321 * Pm + t) / z
        tol = dict(u=S.K[0] * geo * (1 + np.abs(w["u"] - S.K[2]) / S.K[0]) + 4 * eps * (np.abs(w["u"]) + S.K[2]),
                   v=S.K[1] * geo * (1 + np.abs(w["v"] - S.K[3]) / S.K[1]) + 4 * eps * (np.abs(w["v"]) + S.K[3]))
        tol["ur"] = tol["u"] + 4 * eps * (np.abs(w["u"]) + S.BF / z)
        tol["view_cos"] = eps * (2 + 2 * 1.7321 * (Pm + Om) / w["dist"])
        for k in worst:
            gap = np.abs(r["rows"][k].astype(np.float64) - w[k])[ok]
            assert np.all(gap <= tol[k][ok]), (k, gap.max(), (gap / tol[k][ok]).max())
            worst[k] = max(worst[k], float((gap / tol[k][ok]).max()))
        ratio = np.asarray(table.max_distance[idx], np.float64) / w["dist"]
        tab = S.level_table().astype(np.float64)
        clear = ok & (np.abs(ratio[:, None] / tab[None, :] - 1).min(axis=1) > 4 * eps)
        assert np.array_equal(r["rows"]["level"][clear], (tab[None, :] < ratio[clear, None]).sum(axis=1))
        checked += int(clear.sum())
    print("numpy vs restatement, largest gap as a fraction of the format bound: " + ", ".join("%s %.2f" % kv for kv in worst.items()) +
          "; levels checked %d" % checked)
    assert checked > 80


@pytest.mark.parametrize("scale_factor,n_levels", [(1.2, 8), (2.0, 4)])
def test_threshold_table_equals_the_formula(scale_factor, n_levels):
    """The device's rule (count the table entries strictly below the ratio) against ceil(log(ratio) / logScaleFactor), clamped, by this
    machine's libm: every float within 4096 ulp of each threshold and a million random ratios in [0.05, 20].  No mismatch allowed."""
    tab = S.level_table(scale_factor, n_levels)
    assert len(tab) == n_levels - 1 and np.all(np.diff(tab) > 0) and tab[0] == 1.0
    near = np.concatenate([(np.int64(t.view(np.uint32)) + np.arange(-4096, 4097)).astype(np.uint32).view(f32) for t in tab])
    rng = np.random.default_rng(17)
    rand = np.exp(rng.uniform(np.log(0.05), np.log(20.0), 1_000_000)).astype(f32)
    for ratios in (near, rand):
        want, got = S.formula_levels(ratios, scale_factor, n_levels), S.table_levels(ratios, tab)
        assert np.array_equal(got, want), int((got != want).sum())
        assert set(want.tolist()) == set(range(n_levels))
    # each threshold is the LAST float of its level
    for k, t in enumerate(tab):
        up = np.nextafter(t, f32(np.inf))
        assert S.formula_levels([t, up], scale_factor, n_levels).tolist() == [k, k + 1]


def test_thresholds_of_the_default_pyramid():
    tab = S.level_table(1.2, 8)
    assert [float(x) for x in tab[:3]] == [1.0, float(f32(1.20000005)), float(f32(1.44000006))]


def test_both_clamps_and_the_undefined_conversions():
    tab = S.level_table(1.2, 8)
    ratios = np.array([1e-30, 0.5, 1.0, 3.6, 100.0, 3e38, np.inf, np.nan, 0.0, -1.0], f32)
    want = [0, 0, 0, 7, 7, 7, 7, 0, 0, 0]
    assert S.table_levels(ratios, tab).tolist() == want
    assert S.formula_levels(ratios, 1.2, 8).tolist() == want
    assert S.level_table(1.2, 1).size == 0 and S.table_levels(ratios, S.level_table(1.2, 1)).tolist() == [0] * len(ratios)


def test_scene_takes_every_exit_and_level():
    """The GPU tests' batch, on the restatement: every exit 0-6 and every level 0-7 occurs."""
    views, logs, table, lists, skips = S.scene()
    res = S.ref_cull(views, logs, table, lists, skips)
    st = np.concatenate([r["status"] for r in res])
    lv = np.concatenate([r["rows"]["level"][r["status"] == 0] for r in res])
    assert set(st.tolist()) == set(range(7)) and set(lv.tolist()) == set(range(8))
    assert [r["n_in_view"] for r in res] == [int((r["status"] == 0).sum()) for r in res]


def test_tracking_adapter_typechecks():
    H = os.path.join(ROOT, "tests", "cpu_harness")
    subprocess.check_call(["g++", "-std=c++14", "-fsyntax-only", "-I" + os.path.join(H, "mock"), os.path.join(H, "tracking_syntax_check.cpp")])


def test_abi_rejects_bad_arguments_without_a_gpu():
    """List, index and level errors are reported before any device work, so this runs anywhere."""
    import ydorbslam_amd as y
    from ydorbslam_amd.frustum import FrustumBatch, frustum_cull
    y.build_library()
    views, logs, table, lists, skips = S.scene()
    L = y.lib()

    def rejected(match, views=views, table=table, lists=lists, skips=skips):
        with pytest.raises(y.YdorbError, match=match):
            frustum_cull(views, table, lists, skips)

    rejected("point index", lists=[[table.n], [], []], skips=[[0], [], []])
    rejected("point index", lists=[[-1], [], []], skips=[[0], [], []])
    for bad_levels in (0, 9):
        v, _ = S.view(*S.pose())
        v.n_levels = bad_levels
        rejected("n_levels", views=[views[0], v, views[2]])
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    B = FrustumBatch(views, table, lists, skips)
    rows, status, n_in = B.outputs()
    assert L.ydorb_frustum_cull(None, p(rows), p(status), p(n_in)) == -1
    assert L.ydorb_frustum_cull(C.byref(B.struct), None, p(status), p(n_in)) == -1 and b"null list or output" in L.ydorb_last_error()
    B.start[1] = -1
    assert L.ydorb_frustum_cull(C.byref(B.struct), p(rows), p(status), p(n_in)) == -1 and b"non-decreasing" in L.ydorb_last_error()
    B.start[1] = int(B.start[2])
    B.start[0] = 1
    assert L.ydorb_frustum_cull(C.byref(B.struct), p(rows), p(status), p(n_in)) == -1 and b"list_start[0]" in L.ydorb_last_error()
    B.start[0] = 0
    B.struct.table.pos_min = None
    assert L.ydorb_frustum_cull(C.byref(B.struct), p(rows), p(status), p(n_in)) == -1 and b"map-point table" in L.ydorb_last_error()
    B.struct.table.pos_min = p(table.pos_min)
    B.struct.device = 16
    assert L.ydorb_frustum_cull(C.byref(B.struct), p(rows), p(status), p(n_in)) == -1
    assert L.ydorb_frustum_release(-1) == -1
    # the fused call checks its own arguments before it touches the handle's device
    v = views[0]
    n_to, n_m = C.c_int32(0), C.c_int32(0)
    assert L.ydorb_search_local_points(None, None, C.byref(v), C.byref(table.struct), None, None, 1.0, 0.8, None, None, None, None,
                                       C.byref(n_to), C.byref(n_m)) == -1
