"""Shared inputs of the BA tests that make the LM loop REJECT steps (test_ba_lm_paths_cpu.py, test_ba_lm_paths_gpu.py).

synth_ba_problem starts 5 mm / 3 cm from the truth: every LM step is accepted, one trial per outer iteration.  hard_ba_problem
pushes the free poses and the points metres away, so that steps are rejected, lambda grows, a stage ends on max_trials, every edge
is culled, or a stage ends early.  ROWS names the inputs and what the CPU oracle does on each.
"""
import numpy as np

from ydorbslam_amd.synth import synth_ba_problem


def hard_ba_problem(K, P, O, synth_kwargs, seed, pose_sigma, point_sigma):
    """synth_ba_problem(K, P, O, **synth_kwargs) with the free poses' translations and all points perturbed, in this order, from
    default_rng(seed)."""
    base = synth_ba_problem(K, P, O, **synth_kwargs)
    rng = np.random.default_rng(seed)
    free = base["fixed"] == 0
    base["poses"][free, :3] += rng.normal(0, pose_sigma, (int(free.sum()), 3))
    base["points"] += rng.normal(0, point_sigma, base["points"].shape)
    return base


def trials_per_iteration(log):
    return [int(t) for t in log[:, 2]]


def decisions_are_stable(oracle, prob, options, eps=1e-11, n=6):
    """Do the oracle's integer decisions survive a relative input perturbation of eps?  Solves prob and n copies whose poses and
    points are multiplied by 1 + eps * N(0, 1) (default_rng(100 + s)).  Returns (all runs agree on the trial count, log[:, 2:] and
    the outlier mask; largest relative spread of log[:, 0] over the runs).  It stands in for "another summation order": an input
    whose decisions flip under 1e-11 cannot be compared with another implementation at all."""
    ref = oracle.ba_solve(prob, options)
    stable, spread = True, 0.0
    for s in range(n):
        rng = np.random.default_rng(100 + s)
        q = dict(prob)
        q["poses"] = prob["poses"] * (1 + eps * rng.normal(size=prob["poses"].shape))
        q["points"] = prob["points"] * (1 + eps * rng.normal(size=prob["points"].shape))
        r = oracle.ba_solve(q, options)
        same = (r["trials"] == ref["trials"] and r["log"].shape == ref["log"].shape and np.array_equal(r["log"][:, 2:], ref["log"][:, 2:])
                and np.array_equal(r["outlier"], ref["outlier"]))
        stable = stable and same
        if same and len(ref["log"]):
            spread = max(spread, float(np.max(np.abs(r["log"][:, 0] - ref["log"][:, 0]) / np.abs(ref["log"][:, 0]))))
    return stable, spread


# name -> hard_ba_problem arguments
PROBLEMS = {
    "A": (5, 150, 4, dict(seed=3), 1, 1.0, 2.0),
    "B": (8, 200, 4, dict(seed=20, outlier_frac=0.05), 2, 1.0, 2.0),
    "C": (6, 120, 4, dict(seed=3, mono_frac=1.0), 3, 1.0, 2.0),
    "D": (4, 30, 3, dict(seed=32), 4, 1.3, 2.5),
    "E": (9, 300, 5, dict(seed=33, n_fixed=3, mono_frac=0.5), 1, 1.0, 2.0),
    "F": (5, 150, 4, dict(seed=3), 1, 2.0, 4.0),
    "G": (6, 120, 4, dict(seed=3, mono_frac=1.0), 1, 1.0, 2.0),
}

# option specs: ("local", max_trials) is localBundleAdjust's two-stage schedule, ("global", iters, robust) is bundleAdjust's one stage
LOCAL = ("local", 10)
LOCAL_2 = ("local", 2)
GLOBAL_R = ("global", 8, True)
GLOBAL_N = ("global", 8, False)

# (id, problem, options): every row whose oracle decisions are stable (tests/test_ba_lm_paths_cpu.py asserts that)
STABLE_ROWS = [
    ("A-local", "A", LOCAL), ("A-global-robust", "A", GLOBAL_R), ("A2-local-max2", "A", LOCAL_2),
    ("B-local", "B", LOCAL), ("B-global-plain", "B", GLOBAL_N),
    ("C-local", "C", LOCAL), ("C-global-robust", "C", GLOBAL_R),
    ("D-local", "D", LOCAL), ("D-global-plain", "D", GLOBAL_N), ("D-global-robust", "D", GLOBAL_R),
    ("E-global-robust", "E", GLOBAL_R),
    ("F-local", "F", LOCAL),
]
UNSTABLE_ROW = ("G-local", "G", LOCAL)

_cache = {}


def problem(name):
    """The named input; built once, callers must not write into it."""
    if name not in _cache:
        _cache[name] = hard_ba_problem(*PROBLEMS[name])
        for v in _cache[name].values():
            v.setflags(write=False)
    return _cache[name]


def oracle_options(oracle, spec):
    if spec[0] == "local":
        o = oracle.ba_default_options()
        o["max_trials"] = spec[1]
        return o
    return oracle.ba_global_options(spec[1], spec[2])


def gpu_options(spec, extra_flags=0):
    import ydorbslam_amd as y
    if spec[0] == "local":
        o = y.Optimizer.default_options()
        o.max_trials = spec[1]
    else:
        o = y.Optimizer.global_options(spec[1], spec[2])
    o.flags |= extra_flags
    return o


_oracle_cache = {}


def oracle_solve(oracle, name, spec):
    """The oracle's solve of a row, computed once per session and shared (read-only)."""
    key = (name, spec)
    if key not in _oracle_cache:
        r = oracle.ba_solve(problem(name), oracle_options(oracle, spec))
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _oracle_cache[key] = r
    return _oracle_cache[key]


def check_against_oracle(ref, got):
    """GPU solve against the oracle's: tolerance as BASELINE.md states it - chi2 and lambda per outer iteration within 1e-6 relative,
    trial counts, stages and the outlier mask (integer decisions) identical, poses / points within 1e-4 relative on the float32
    values Converter hands back."""
    assert got["trials"] == ref["trials"]
    assert len(got["log"]) == len(ref["log"])
    assert np.allclose(got["log"][:, 0], ref["log"][:, 0], rtol=1e-6, atol=0)       # chi2 per outer iteration
    assert np.allclose(got["log"][:, 1], ref["log"][:, 1], rtol=1e-6, atol=0)       # lambda
    assert np.array_equal(got["log"][:, 2:], ref["log"][:, 2:])                     # trials, stage
    assert np.array_equal(got["outlier"], ref["outlier"])
    p32, r32 = got["poses"].astype(np.float32), ref["poses"].astype(np.float32)     # what Converter hands back (float cv::Mat)
    assert np.allclose(p32, r32, rtol=1e-4, atol=1e-6)
    assert np.allclose(got["points"].astype(np.float32), ref["points"].astype(np.float32), rtol=1e-4, atol=1e-6)


def same_bytes(a, b):
    """Two solves of the wrapper agree byte for byte: poses, points, outlier mask, trial count and the whole log."""
    return (a["poses"].tobytes() == b["poses"].tobytes() and a["points"].tobytes() == b["points"].tobytes()
            and np.array_equal(a["outlier"], b["outlier"]) and a["trials"] == b["trials"] and a["iterations"] == b["iterations"]
            and a["log"].tobytes() == b["log"].tobytes() and a["stopped"] == b["stopped"])
