"""The essential graph's block-skyline solver without a GPU: the host plan (ydorbslam_amd/csrc/skyline_plan.h) in a
stand-alone program under the address and undefined-behaviour sanitizers and through ydorb_essential_graph_plan, which touches no
device; the skyline restatement against the dense one, byte for byte; the new host program's syntax."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import essgraph_skyline_support as K
import essgraph_support as S
from essgraph_support import ROOT

PLAN_SRC = os.path.join(ROOT, "tests", "cpu_harness", "skyline_plan_check.cpp")
PLAN_HEADER = os.path.join(ROOT, "ydorbslam_amd", "csrc", "skyline_plan.h")
DEFAULT_LIMIT = 19200 * 19200 * 8


def test_plan_properties_in_a_sanitized_program(tmp_path):
    """perm is a permutation, every free edge lies inside the envelope, first[f] <= f and is attained, the column lists are ascending and
    match first, SMALLER is never larger than NATURAL (natural on a tie), a ring under RCM has rows of at most 3 blocks (n = 12, 101),
    two calls give identical arrays: on two, six, ring12 with repeated pairs, tree40, both stars, two components, a fixed vertex in
    mid-numbering and two fixed vertices.  Then, for 6x6 and 7x7 blocks on a closed ring of 12 and a star of 5 with the hub first under
    the natural and the RCM plan: an envelope of distinct values expands to a symmetric matrix that is zero outside the envelope under
    both conventions for the diagonal blocks, and packing the expansion returns the envelope's bytes (failures only are printed).  The
    program is its own process; nothing is loaded into this one."""
    exe = str(tmp_path / "skyline_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", PLAN_SRC, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.splitlines()
    assert lines[-1] == "0 failed" and len(lines) == 12
    assert any(l.startswith("tree40") and l.endswith("rcm") for l in lines)
    assert any(l.startswith("star, hub last") and l.endswith("natural") for l in lines)


def test_plan_header_has_no_hip():
    text = open(PLAN_HEADER).read()
    assert "#include <hip" not in text and "hipStream" not in text and "__global__" not in text and "__device__" not in text


def _plan(g, **kw):
    from ydorbslam_amd.essential_graph import plan
    return plan(g["sim3"], g["fixed"], g["edges"], g["meas"], fix_scale=g["fix_scale"], **kw)


PLAN_GRAPHS = {
    "two": lambda: K.plain_graph(2, [(0, 1)]),
    "six": lambda: K.plain_graph(6, S.ring(6, chords=[(1, 4)])),
    "ring12": lambda: K.plain_graph(12, S.ring(12, repeated=[(3, 4), (4, 3)])),
    "tree40": lambda: K.plain_graph(40, S.tree40()),
    "star_first": lambda: K.plain_graph(10, [(0, 1)] + [(1, v) for v in range(2, 10)]),
    "star_last": lambda: K.plain_graph(10, [(0, 9)] + [(v, 9) for v in range(1, 9)]),
    "components": lambda: K.plain_graph(8, [(0, 1), (1, 2), (2, 3), (3, 1), (0, 4), (4, 5), (5, 6), (6, 7), (7, 4)]),
    "fixed_middle": lambda: K.plain_graph(9, S.ring(9, chords=[(2, 6)]), fixed=(4,)),
    "two_fixed": lambda: K.plain_graph(11, S.ring(11, chords=[(1, 8), (5, 0), (5, 7)]), fixed=(0, 7)),
}


@pytest.mark.parametrize("name", sorted(PLAN_GRAPHS))
def test_library_plans_without_a_device(name):
    """ydorb_essential_graph_plan is host code: it answers here, where no GPU is required, with the properties of the stand-alone check."""
    import ydorbslam_amd as y
    y.build_library()
    g = PLAN_GRAPHS[name]()
    plans = {o: _plan(g, solver="skyline", ordering=o) for o in ("natural", "rcm", "smaller")}
    for o, p in plans.items():
        K.check_plan(g, p)
        assert p["solver_used"] == "skyline" and p["factor_bytes"] == 392 * p["envelope_blocks"]
        again = _plan(g, solver="skyline", ordering=o)
        assert np.array_equal(again["perm"], p["perm"]) and np.array_equal(again["first"], p["first"])
    nat, rcm, small = plans["natural"], plans["rcm"], plans["smaller"]
    assert nat["ordering_used"] == "natural" and np.array_equal(nat["perm"], np.arange(nat["n_free"])) and rcm["ordering_used"] == "rcm"
    assert small["envelope_blocks"] == min(nat["envelope_blocks"], rcm["envelope_blocks"]) <= nat["envelope_blocks"]
    assert small["ordering_used"] == ("rcm" if rcm["envelope_blocks"] < nat["envelope_blocks"] else "natural")
    # AUTO below the dense limit is the dense solver; the envelope is still reported
    auto = _plan(g)
    padded = (7 * auto["n_free"] + 31) // 32 * 32
    assert auto["solver_used"] == "dense" and auto["factor_bytes"] == padded * padded * 8 and auto["envelope_blocks"] == small["envelope_blocks"]


@pytest.mark.parametrize("n", [12, 101])
def test_ring_under_rcm_is_a_band(n):
    g = K.plain_graph(n + 1, S.ring(n), fixed=(n,))   # the ring closes among free vertices
    nat, rcm = _plan(g, solver="skyline", ordering="natural"), _plan(g, solver="skyline", ordering="rcm")
    assert nat["max_row_blocks"] == n and rcm["max_row_blocks"] <= 3


def test_plan_rejects_what_optimize_rejects():
    import ydorbslam_amd as y
    from ydorbslam_amd._lib import YdBaResult, YdEssentialSolverInfo, YdEssentialSolverOptions
    from ydorbslam_amd.essential_graph import EssentialGraph
    y.build_library()
    L = y.lib()
    g = S.solve_graph("six", True)
    info, res = YdEssentialSolverInfo(), YdBaResult()
    sky = YdEssentialSolverOptions(2, 0, 0)

    def both(G, opt=sky, out=None):
        """the plan's answer and optimize_with's, which must agree on every argument error (neither reaches a device for one)"""
        a = L.ydorb_essential_graph_plan(C.byref(G.struct), C.byref(opt), C.byref(info), None, None)
        text = L.ydorb_last_error()
        b = L.ydorb_essential_graph_optimize_with(C.byref(G.struct), C.byref(opt), out, C.byref(res), None)
        assert a == b and text == L.ydorb_last_error(), (a, b, text, L.ydorb_last_error())
        return a, text

    def graph(**kw):
        d = dict(sim3=g["sim3"], fixed=g["fixed"], edges=g["edges"], meas=g["meas"])
        d.update(kw)
        return EssentialGraph(**d)

    def rejected(text, **kw):
        rc, got = both(graph(**kw))
        assert rc == -1 and text in got, got

    assert L.ydorb_essential_graph_plan(None, C.byref(sky), C.byref(info), None, None) == -1
    assert L.ydorb_essential_graph_plan(C.byref(graph().struct), C.byref(sky), None, None, None) == -1
    for field in ("sim3", "fixed", "edge_v0", "edge_v1", "edge_meas"):
        G = graph()
        setattr(G.struct, field, None)
        rc, text = both(G)
        assert rc == -1 and b"null array" in text
    pts = np.zeros((3, 3), np.float32)
    G = graph(points=pts, point_ref=[0, 6, 2])
    rc, text = both(G, out=pts.ctypes.data_as(C.c_void_p))
    assert rc == -1 and b"point 1 references" in text
    for bad in (-1, 6):
        e = g["edges"].copy()
        e[2, 1] = bad
        rejected(b"edge 2 references", edges=e)
    e = g["edges"].copy()
    e[3] = (4, 4)
    rejected(b"to itself", edges=e)
    rejected(b"no fixed vertex", fixed=np.zeros(6, np.uint8))
    rejected(b"every vertex is fixed", fixed=np.ones(6, np.uint8))
    rejected(b"iterations", iterations=0)
    rejected(b"iterations", max_trials=0)
    rejected(b"lambda_init", lambda_init=0.0)
    s = g["sim3"].copy()
    s[4, 7] = 0.0
    rejected(b"vertex 4 has a non-positive scale", sim3=s)
    m = g["meas"].copy()
    m[1, 7] = -1.0
    rejected(b"edge 1 has a non-positive scale", meas=m)
    G = graph()
    G.struct.device = 16
    assert both(G)[0] == -1
    for opt, text in ((YdEssentialSolverOptions(3, 0, 0), b"unknown solver"), (YdEssentialSolverOptions(2, 3, 0), b"unknown ordering"),
                      (YdEssentialSolverOptions(2, 0, -1), b"max_factor_bytes")):
        rc, got = both(graph(), opt)
        assert rc == -1 and text in got
    # the trial step's copies of the system are for small graphs
    big = K.plain_graph(590, S.ring(590))
    G = EssentialGraph(big["sim3"], big["fixed"], big["edges"], big["meas"])
    x, solved, H = np.zeros(7 * 589), C.c_int32(0), np.zeros(1)
    assert L.ydorb_essential_graph_trial_step_with(C.byref(G.struct), C.byref(sky), 1.0, x.ctypes.data_as(C.c_void_p), C.byref(solved),
                                                   H.ctypes.data_as(C.c_void_p), None) == -1 and b"4096 rows" in L.ydorb_last_error()


def test_size_limits_name_the_solver_they_belong_to():
    """DENSE keeps its 2 742 free vertices (same code, same text as the old entry); AUTO goes to the skyline above it; the skyline's limit
    is the envelope's bytes: a 30 000-vertex star with the hub first is dense in natural order, 176 GB, and a band of two under RCM."""
    import ydorbslam_amd as y
    from ydorbslam_amd._lib import YdorbError
    y.build_library()
    L = y.lib()
    chain = K.plain_graph(2744, [(i, i + 1) for i in range(2743)])
    with pytest.raises(YdorbError, match="ydorb error -5.*at most 2742"):
        _plan(chain, solver="dense")
    # the old trial step names the dense limit before it looks at lambda or its outputs, as it always did
    from ydorbslam_amd.essential_graph import EssentialGraph
    G = EssentialGraph(chain["sim3"], chain["fixed"], chain["edges"], chain["meas"])
    assert L.ydorb_essential_graph_trial_step(C.byref(G.struct), 0.0, None, None) == -5 and b"at most 2742" in L.ydorb_last_error()
    auto = _plan(chain)
    assert auto["solver_used"] == "skyline" and auto["n_free"] == 2743 and auto["envelope_blocks"] == 2 * 2743 - 1 and auto["max_row_blocks"] == 2
    n = 30000
    star = K.plain_graph(n, [(0, 1)] + [(1, v) for v in range(2, n)])
    nf = n - 1
    dense_blocks = nf * (nf + 1) // 2
    with pytest.raises(YdorbError) as err:
        _plan(star, solver="skyline", ordering="natural")
    text = str(err.value)
    assert "ydorb error -5" in text and str(dense_blocks * 392) in text and str(DEFAULT_LIMIT) in text, text
    # DENSE does not apply the envelope's limit, this graph fails the dense one; AUTO above the dense limit is SKYLINE and does apply it
    with pytest.raises(YdorbError, match="at most 2742"):
        _plan(star, solver="dense", ordering="natural")
    with pytest.raises(YdorbError, match="takes %d bytes" % (dense_blocks * 392)):
        _plan(star, solver="auto", ordering="natural")
    assert _plan(star, solver="auto")["solver_used"] == "skyline"
    small = _plan(star, solver="skyline", ordering="smaller")
    K.check_plan(star, small)
    assert small["ordering_used"] == "rcm" and small["envelope_blocks"] == 2 * nf - 1 and small["envelope_blocks_natural"] == dense_blocks
    assert small["factor_bytes"] <= DEFAULT_LIMIT
    # the caller may move the limit either way (a star small enough for its dense envelope to be planned: 20 100 blocks)
    star = K.plain_graph(201, [(0, 1)] + [(1, v) for v in range(2, 201)])
    with pytest.raises(YdorbError, match="takes %d bytes.*max_factor_bytes is 1000000" % (20100 * 392)):
        _plan(star, solver="skyline", ordering="natural", max_factor_bytes=1000000)
    raised = _plan(star, solver="skyline", ordering="natural", max_factor_bytes=20100 * 392)
    assert raised["ordering_used"] == "natural" and raised["factor_bytes"] == 20100 * 392
    # the bytes bound the memory, a second limit the work of the one workgroup: a dense envelope of 601 block rows is 71 MB, well inside
    # the default bytes, and 600 * 601 * 602 / 6 = 36 180 200 block updates per trial, above 2^24; the band RCM makes of it is not
    star = K.plain_graph(602, [(0, 1)] + [(1, v) for v in range(2, 602)])
    with pytest.raises(YdorbError, match="ydorb error -5.*takes 36180200 block updates.*at most 16777216"):
        _plan(star, solver="skyline", ordering="natural")
    assert _plan(star, solver="skyline", ordering="smaller")["envelope_blocks"] == 2 * 601 - 1
    assert L.ydorb_device_count() >= 0


@pytest.mark.parametrize("fix_scale", [True, False])
@pytest.mark.parametrize("shape", S.SOLVE_SHAPES)
def test_skyline_restatement_equals_the_dense_one_byte_for_byte(shape, fix_scale):
    g = S.solve_graph(shape, fix_scale)
    pts, ref = S.map_points(33, g["n"], 7, always=(0,))
    a, b = S.ref_optimize(g, pts, ref), K.sky_ref_optimize(g, pts, ref)
    for key in ("sim3", "log_chi2", "log_lambda", "log_trials", "points", "points_d"):
        assert a[key].tobytes() == b[key].tobytes(), key
    assert a["n_trials"] == b["n_trials"] and a["n_iterations"] == b["n_iterations"]
    n = 7 * int((g["fixed"] == 0).sum())
    assert 0 < b["skyline_doubles"] <= n * (n + 1) // 2


def test_skyline_restatement_rejects_trials_like_the_dense_one():
    g = S.far_start_graph()
    a, b = S.ref_optimize(g, **S.FAR), K.sky_ref_optimize(g, **S.FAR)
    assert a["log_trials"].tolist() == b["log_trials"].tolist() == [9, 1, 1]
    assert a["sim3"].tobytes() == b["sim3"].tobytes() and a["log_lambda"].tobytes() == b["log_lambda"].tobytes()


def test_skyline_host_program_typechecks():
    H = os.path.join(ROOT, "tests", "cpu_harness")
    subprocess.check_call(["g++", "-std=c++14", "-fsyntax-only", "-I" + os.path.join(H, "mockrt"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp_host", "essgraph_skyline_run.cpp")])
