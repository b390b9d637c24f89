"""The BA's block-skyline reduced camera solve without a GPU: the host plan (ydorbslam_amd/csrc/ba_pairs.h) in a
stand-alone program under the address and undefined-behaviour sanitizers, and through ydorb_ba_plan, which touches no device, against
a numpy statement of the pair list and the envelope."""
import os
import subprocess

import numpy as np
import pytest

import ba_skyline_support as K
from ba_skyline_support import ROOT

SRC = os.path.join(ROOT, "tests", "cpu_harness", "ba_pairs_check.cpp")
HEADER = os.path.join(ROOT, "ydorbslam_amd", "csrc", "ba_pairs.h")
DEFAULT_LIMIT = 19200 * 19200 * 8
NATURAL, RCM, SMALLER = 1, 2, 0
AUTO, DENSE, SKYLINE = 0, 1, 2


@pytest.fixture(scope="module")
def opt():
    import ydorbslam_amd as y
    y.build_library()
    return y.Optimizer


def test_pair_list_and_plan_in_a_sanitized_program(tmp_path):
    """Each pair once and ordered, every bucket found by the search the device uses, perm a permutation, first and the sizes equal to a
    brute-force statement, every bucket's destination inside its row and transposed exactly when the order swaps the pair, column lists
    ascending; both refusals carry both figures and come before the column lists.  The program is its own process."""
    exe = str(tmp_path / "ba_pairs_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", SRC, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.splitlines()
    assert lines[-1] == "0 failed" and len(lines) == 13
    assert any(l.startswith("loop, smaller") and l.endswith("rcm") for l in lines)


def test_plan_header_has_no_hip():
    text = open(HEADER).read()
    assert "#include <hip" not in text and "hipStream" not in text and "__global__" not in text and "__device__" not in text


def _star(n):
    """keyframe 1 sees every point, every other free keyframe one of them"""
    return K.graph_problem(n + 1, [[1, k] for k in range(2, n + 1)])


GRAPHS = {
    "chain": lambda: K.trajectory_problem(30, span=3, per_kf=2),
    "loop": lambda: K.trajectory_problem(40, span=3, per_kf=2, loop=True),
    "star": lambda: _star(25),
    "components": lambda: K.graph_problem(7, [[0, 1], [1, 2], [2, 3], [4, 5], [5, 6], [4, 6]]),
    "fixed_only": lambda: K.graph_problem(6, [[1, 2], [0, 3, 4], [2, 1]], fixed=(0, 4)),     # keyframe 3 shares points with fixed ones only
    "idle": lambda: K.graph_problem(6, [[1, 2], [2, 4], [4, 5]]),                             # keyframe 3 has no edge
    "all_fixed": lambda: K.graph_problem(4, [[0, 1, 2], [2, 3]], fixed=(0, 1, 2, 3)),
}


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_plan_against_numpy(opt, name):
    prob = GRAPHS[name]()
    plans = {o: opt.plan(prob, solver=SKYLINE, ordering=o) for o in (NATURAL, RCM, SMALLER)}
    for o, p in plans.items():
        K.check_plan(prob, p)
        assert p["solver_used"] == SKYLINE and p["factor_bytes"] == 288 * p["envelope_blocks"] and p["dense_max_rows"] == 19200
        again = opt.plan(prob, solver=SKYLINE, ordering=o)
        assert np.array_equal(again["perm"], p["perm"]) and np.array_equal(again["first"], p["first"])
    nat, rcm, small = plans[NATURAL], plans[RCM], plans[SMALLER]
    n = nat["n_free"]
    assert nat["ordering_used"] == NATURAL and np.array_equal(nat["perm"], np.arange(n)) and rcm["ordering_used"] == RCM
    assert small["envelope_blocks"] == min(nat["envelope_blocks"], rcm["envelope_blocks"])
    assert small["ordering_used"] == (RCM if rcm["envelope_blocks"] < nat["envelope_blocks"] else NATURAL)
    auto = opt.plan(prob)                      # AUTO below the dense limit is the dense solver; the envelope is still reported
    padded = max(32, (6 * n + 31) // 32 * 32)
    assert auto["solver_used"] == DENSE and auto["factor_bytes"] == padded * padded * 8 and auto["envelope_blocks"] == small["envelope_blocks"]
    rows = np.arange(n) - nat["first"] + 1
    if name == "chain":
        assert n == 29 and rows.max() == 3 and small["ordering_used"] == NATURAL
    elif name == "loop":
        span = 3
        assert (rows == n).sum() >= 1 and rcm["max_row_blocks"] <= 2 * span and small["ordering_used"] == RCM
    elif name == "star":
        assert nat["envelope_blocks"] == n * (n + 1) // 2 and nat["covisible_pairs"] == n - 1
    elif name == "components":
        assert n == 6 and rows[3] == 1 and rows[2] == 2
    elif name == "fixed_only":
        assert n == 3 and nat["covisible_pairs"] == 1 and rows[2] == 1
    elif name == "idle":
        assert n == 4 and nat["covisible_pairs"] == 3           # keyframes 1, 2, 4, 5
    else:
        assert n == 0 and nat["envelope_blocks"] == 0 and nat["covisible_pairs"] == 0


def test_buckets_grow_with_the_pairs_not_with_the_square(opt):
    """20 000 free poses in a chain of span 2: the dense path would have 200 010 000 buckets; the pair list has one per covisible pair
    and one per pose, the numbers numpy finds, and every size the plan reports doubles when the map does."""
    infos = {}
    for n in (5000, 10000, 20000):
        prob = K.trajectory_problem(n + 1, span=2, per_kf=1)
        p = opt.plan(prob)
        assert p["n_free"] == n and p["solver_used"] == (SKYLINE if 6 * n > 19200 else DENSE)
        assert p["covisible_pairs"] == len(K.numpy_pairs(prob)) == n - 1
        infos[n] = opt.plan(prob, solver=SKYLINE)
    big = infos[20000]
    assert big["factor_bytes"] <= DEFAULT_LIMIT and big["factor_bytes"] == 288 * (2 * 20000 - 1)
    for key in ("covisible_pairs", "envelope_blocks", "pair_updates"):
        assert 2 * (infos[10000][key] - infos[5000][key]) == infos[20000][key] - infos[10000][key], key
        assert infos[20000][key] < 3 * 20000, key


def test_refusals_that_need_no_device(opt):
    from ydorbslam_amd._lib import YdorbError
    prob = K.trajectory_problem(3202, span=2, per_kf=1)        # 3 201 free poses: 19 206 rows, padded to 19 232
    with pytest.raises(YdorbError, match=r"ydorb error -5: reduced camera system of 19232 rows is wider than the solve kernel's LDS \(max 19200\)"):
        opt.plan(prob, solver=DENSE)
    assert opt.plan(prob)["solver_used"] == SKYLINE
    at_limit = K.trajectory_problem(3201, span=2, per_kf=1)
    assert opt.plan(at_limit)["solver_used"] == DENSE and opt.plan(at_limit, solver=DENSE)["factor_bytes"] == DEFAULT_LIMIT
    small = K.trajectory_problem(30, span=3, per_kf=1)
    with pytest.raises(YdorbError, match=r"ydorb error -5.*takes 24192 bytes \(84 blocks, natural order\), max_factor_bytes is 1000"):
        opt.plan(small, solver=SKYLINE, max_factor_bytes=1000)
    assert opt.plan(small, solver=SKYLINE, max_factor_bytes=24192)["envelope_blocks"] == 84
    with pytest.raises(YdorbError, match="ydorb error -5.*one rank"):
        opt.plan(small, solver=SKYLINE, world=2)
    # the work bound: a dense envelope of 602 block rows is 52 MB, inside the default bytes, and 36 361 101 block updates, above 2^24
    star = _star(602)
    with pytest.raises(YdorbError, match="ydorb error -5.*takes 36361101 block updates.*at most 16777216"):
        opt.plan(star, solver=SKYLINE, ordering=NATURAL)
    assert opt.plan(star, solver=SKYLINE)["envelope_blocks"] == 2 * 602 - 1
    for bad, text in (((3, 0, 0), "unknown solver"), ((2, 3, 0), "unknown ordering"), ((2, 0, -1), "max_factor_bytes")):
        with pytest.raises(YdorbError, match=text):
            opt.plan(small, solver=bad[0], ordering=bad[1], max_factor_bytes=bad[2])


def test_adapter_host_program_typechecks():
    H = os.path.join(ROOT, "tests", "cpu_harness")
    subprocess.check_call(["g++", "-std=c++14", "-fsyntax-only", "-I" + os.path.join(H, "mockrt"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp_host", "gba_skyline_run.cpp")])
