"""Shared inputs and references of the BA tests.

First part: inputs that make the LM loop REJECT steps (test_ba_lm_paths_cpu.py, test_ba_lm_paths_gpu.py).

synth_ba_problem starts 5 mm / 3 cm from the truth: every LM step is accepted, one trial per outer iteration.  hard_ba_problem
pushes the free poses and the points metres away, so that steps are rejected, lambda grows, a stage ends on max_trials, every edge
is culled, or a stage ends early.  ROWS names the inputs and what the CPU oracle does on each.

Second part (test_ba_structure_cpu.py, test_ba_structure_gpu.py): realistic_ba_problem, a graph with the structure synth_ba_problem
never has - rotated cameras, per-octave information, ragged observation counts, vertices without edges, fixed keyframes in the
middle, shuffled edges - and two numpy references that share no code with the oracle or the kernels: numpy_chi2 (the objective) and
numpy_lm_first_step (one LM iteration from finite-difference Jacobians and a dense solve).
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
        _cache[name] = STRUCTURE_PROBLEMS[name]() if name in STRUCTURE_PROBLEMS else hard_ba_problem(*PROBLEMS[name])
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


# ------------------------------------------------------------------------------------------------------------------------------------
# Realistic graph structure (test_ba_structure_cpu.py, test_ba_structure_gpu.py)
# ------------------------------------------------------------------------------------------------------------------------------------
def _quat_from_rotvec(w):
    """(x, y, z, w) of the rotation exp([w]x); exact at any angle (no division by the quaternion's w)."""
    th = float(np.linalg.norm(w))
    if th < 1e-12:
        return np.array([0.5 * w[0], 0.5 * w[1], 0.5 * w[2], 1.0])
    return np.concatenate([np.sin(0.5 * th) / th * np.asarray(w, np.float64), [np.cos(0.5 * th)]])


def _quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def quat_to_rot(q):
    """Rotation matrices [..., 3, 3] of quaternions [..., 4] in (x, y, z, w) order, normalised first."""
    q = np.asarray(q, np.float64)
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    Rm = np.empty(q.shape[:-1] + (3, 3))
    Rm[..., 0, 0] = 1 - 2 * (y * y + z * z); Rm[..., 0, 1] = 2 * (x * y - z * w); Rm[..., 0, 2] = 2 * (x * z + y * w)
    Rm[..., 1, 0] = 2 * (x * y + z * w); Rm[..., 1, 1] = 1 - 2 * (x * x + z * z); Rm[..., 1, 2] = 2 * (y * z - x * w)
    Rm[..., 2, 0] = 2 * (x * z - y * w); Rm[..., 2, 1] = 2 * (y * z + x * w); Rm[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return Rm


# what Frame keeps as floats (m_flt_fx ...): not round, fx != fy, every value a float32
REALISTIC_CAMERA = np.array([np.float32(v) for v in (517.306408, 516.469215, 318.643040, 255.313989, 38.7714)], np.float64)
_SCENE_CENTRE = np.array([0.0, 0.0, 6.0])


def _project(Rm, t, X, cam):
    """Pixel (u, v) and depth of world point(s) X in the camera X_c = Rm X + t."""
    Xc = X @ Rm.T + t
    z = Xc[..., 2]
    return cam[0] * Xc[..., 0] / z + cam[2], cam[1] * Xc[..., 1] / z + cam[3], z


def realistic_ba_problem(K=14, P=500, seed=1, fixed=(2, 5, 11), mono_frac=0.3, outlier_frac=0.04, n_unobserved=5, n_fixed_only=8,
                         n_single=10, edgeless=True, pose_sigma=0.005, point_sigma=0.03):
    """A local-BA graph as a map produces it, in synth_ba_problem's dictionary layout (poses X_c = R X_w + t as (t, q), q in
    (x, y, z, w) order).  Everything is drawn from default_rng(seed).

    Cameras: K keyframes on an arc 6 m from the scene centre (0, 0, 6), looking inward; rotation vectors (U(-0.15, 0.15), a_k,
    U(-0.15, 0.15)) with a_k from -0.6 to 0.6 rad about y.  The keyframes `fixed` are fixed and keep their true pose; the others start
    5 mrad / 5 mm off (left perturbation, as synth).  With edgeless=True and at least two free keyframes, the middle free one observes
    nothing.
    Points: uniform in a 5 x 3 x 4 m box about the centre (depth 2.5 m or more in every camera), start 3 cm off.  The first n_unobserved
    have no edge, the next n_fixed_only are seen by fixed keyframes only, the next n_single by ONE free keyframe, in stereo (a single
    monocular observation leaves the point's 3x3 block rank 2); every other point by a uniform number in 2 .. all of the keyframes
    that observe.
    Edges: octave o uniform in 0..7, pixel noise 1.2^o, info float32(1.2^-2o); a share mono_frac monocular (u_right = -1; also where
    u_right would come out negative, which is how the solver tells the two apart); a share outlier_frac 30 px off; measurements rounded
    through float32 (cv::KeyPoint); order shuffled.
    Extra keys: truth_poses, truth_points, octave."""
    rng = np.random.default_rng(seed)
    cam = REALISTIC_CAMERA
    fixed_mask = np.zeros(K, np.uint8)
    fixed_mask[list(fixed)] = 1
    free = [k for k in range(K) if not fixed_mask[k]]
    idle = free[len(free) // 2] if (edgeless and len(free) >= 2) else -1
    angles = np.linspace(-0.6, 0.6, K) if K > 1 else np.zeros(1)
    q_true, R_true, t_true = [], [], []
    for k in range(K):
        w = np.array([rng.uniform(-0.15, 0.15), angles[k], rng.uniform(-0.15, 0.15)])
        q_cw = _quat_from_rotvec(w)                       # camera -> world
        centre = _SCENE_CENTRE - rng.uniform(5.7, 6.3) * quat_to_rot(q_cw)[:, 2]
        q = q_cw * np.array([-1.0, -1.0, -1.0, 1.0])      # world -> camera
        Rm = quat_to_rot(q)
        q_true.append(q); R_true.append(Rm); t_true.append(-Rm @ centre)
    truth_poses = np.concatenate([np.array(t_true), np.array(q_true)], axis=1)
    pts = _SCENE_CENTRE + np.stack([rng.uniform(-2.5, 2.5, P), rng.uniform(-1.5, 1.5, P), rng.uniform(-2.0, 2.0, P)], axis=1)

    seeing = [k for k in range(K) if k != idle]
    seeing_fixed = [k for k in seeing if fixed_mask[k]]
    seeing_free = [k for k in seeing if not fixed_mask[k]]
    ep, eq, meas, octs = [], [], [], []

    def observe(p, k, force_stereo):
        """Appends the edge; False (nothing appended) when stereo was demanded and u_right came out negative."""
        o = int(rng.integers(0, 8))
        sigma = 1.2 ** o
        u, v, z = _project(R_true[k], t_true[k], pts[p], cam)
        u += rng.normal(0, sigma); v += rng.normal(0, sigma)
        stereo = force_stereo or rng.random() >= mono_frac
        ur = u - cam[4] / z
        gross = (not force_stereo) and rng.random() < outlier_frac
        if gross:
            u += rng.normal(0, 30); v += rng.normal(0, 30)
        if force_stereo and np.float32(ur) < 0:
            return False
        if not stereo or np.float32(ur) < 0:
            ur = -1.0
        ep.append(k); eq.append(p); meas.append((u, v, ur)); octs.append(o)
        return True

    for p in range(n_unobserved, P):
        special = p - n_unobserved
        if special < n_fixed_only and seeing_fixed:
            pool, n = seeing_fixed, int(rng.integers(1, len(seeing_fixed) + 1))
        elif special < n_fixed_only + n_single or len(seeing) < 2:
            pool, n = seeing_free or seeing, 1
        else:
            pool, n = seeing, int(rng.integers(2, len(seeing) + 1))
        if n == 1:                                        # the first keyframe, in random order, that sees the point in stereo
            done = False
            for k in rng.permutation(pool):
                done = done or observe(p, int(k), True)
            if not done:
                raise ValueError("point %d has no keyframe with a stereo view" % p)
        else:
            for k in np.sort(rng.choice(pool, n, replace=False)):
                observe(p, int(k), False)
    E = len(ep)
    order = rng.permutation(E)
    poses = truth_poses.copy()
    for k in free:
        d = rng.normal(0, pose_sigma, 6)
        dq = _quat_from_rotvec(d[:3])
        poses[k, :3] = quat_to_rot(dq) @ truth_poses[k, :3] + d[3:]
        poses[k, 3:] = _quat_mul(dq, truth_poses[k, 3:])
    points = pts + rng.normal(0, point_sigma, (P, 3))
    octs = np.array(octs, np.int64)[order]
    return dict(poses=poses, fixed=fixed_mask, points=points, edge_pose=np.array(ep, np.int32)[order], edge_point=np.array(eq, np.int32)[order],
                meas=np.array(meas, np.float64).reshape(E, 3)[order].astype(np.float32).astype(np.float64),
                info=(1.0 / 1.2 ** (2 * octs)).astype(np.float32).astype(np.float64), camera=cam.copy(), truth_poses=truth_poses,
                truth_points=pts, octave=octs)


N_BACKFACING = 12


def with_backfacing_camera(prob, fixed, seed=0):
    """prob plus one keyframe (the last index) near (0, 0, 1) turned 0.999 pi about y, so that the whole scene lies BEHIND it, and
    N_BACKFACING monocular edges (the last ones) from it to the points with the most observations.  Each measurement is the exact
    projection through the negative depth, so the edges' chi2 is small and only isDepthPositive can flag them.  fixed=False: the new
    keyframe is free and starts 5 mrad / 5 mm off like the others (default_rng(seed))."""
    q = _quat_from_rotvec(np.array([0.0, 0.999 * np.pi, 0.0])) * np.array([-1.0, -1.0, -1.0, 1.0])
    Rm = quat_to_rot(q)
    t = -Rm @ np.array([0.02, -0.01, 1.0])
    truth = np.concatenate([t, q])
    start = truth.copy()
    if not fixed:
        d = np.random.default_rng(seed).normal(0, 0.005, 6)
        dq = _quat_from_rotvec(d[:3])
        start[:3] = quat_to_rot(dq) @ t + d[3:]
        start[3:] = _quat_mul(dq, q)
    K = len(prob["poses"])
    counts = np.bincount(prob["edge_point"], minlength=len(prob["points"]))
    targets = np.argsort(-counts, kind="stable")[:N_BACKFACING]
    u, v, z = _project(Rm, t, prob["truth_points"][targets], prob["camera"])
    assert (z < -1.0).all()
    meas = np.stack([u, v, -np.ones(N_BACKFACING)], axis=1).astype(np.float32).astype(np.float64)
    out = dict(prob)
    out["poses"] = np.concatenate([prob["poses"], start[None]])
    out["truth_poses"] = np.concatenate([prob["truth_poses"], truth[None]])
    out["fixed"] = np.concatenate([prob["fixed"], [1 if fixed else 0]]).astype(np.uint8)
    out["edge_pose"] = np.concatenate([prob["edge_pose"], np.full(N_BACKFACING, K, np.int32)])
    out["edge_point"] = np.concatenate([prob["edge_point"], targets.astype(np.int32)])
    out["meas"] = np.concatenate([prob["meas"], meas])
    out["info"] = np.concatenate([prob["info"], np.ones(N_BACKFACING)])
    out["octave"] = np.concatenate([prob["octave"], np.zeros(N_BACKFACING, np.int64)])
    return out


def with_duplicated_edges(prob, n=10):
    """prob with its first n edges appended once more: n (pose, point) pairs that occur twice, which no map can produce."""
    out = dict(prob)
    for k in ("edge_pose", "edge_point", "meas", "info"):
        out[k] = np.concatenate([prob[k], prob[k][:n]])
    return out


# ---- numpy references: float64, nothing from oracle/ ---------------------------------------------------------------------------------
def _residuals(Rm, t, X, meas, cam):
    """e[E, 3] = z - projection (EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ; third row 0 for a monocular edge) and the depths, for
    per-edge rotations Rm[E, 3, 3], translations t[E, 3] and points X[E, 3]."""
    Xc = np.einsum("eij,ej->ei", Rm, X) + t
    z = Xc[:, 2]
    u = cam[0] * Xc[:, 0] / z + cam[2]
    v = cam[1] * Xc[:, 1] / z + cam[3]
    stereo = meas[:, 2] >= 0
    e = np.stack([meas[:, 0] - u, meas[:, 1] - v, np.where(stereo, meas[:, 2] - (u - cam[4] / z), 0.0)], axis=1)
    return e, z


def numpy_depths(prob, poses, points):
    """Depth of every edge's point in its keyframe at the estimate (poses, points)."""
    ep, eq = prob["edge_pose"], prob["edge_point"]
    return _residuals(quat_to_rot(poses[:, 3:])[ep], poses[ep, :3], points[eq], prob["meas"], prob["camera"])[1]


def numpy_chi2(prob, poses, points, robust, delta_mono, delta_stereo):
    """The BA objective at (poses, points): sum over ALL edges of info * |e|^2, through Huber's rho (delta per edge kind) when robust.
    Returns (total, per-edge info * |e|^2 without the kernel: the value the chi2 test of the cull compares with 5.991 / 7.815).  The
    deltas are those of the options in use: sqrt(5.991), sqrt(7.815) as floats for local BA, sqrt(5.99) for the mono delta of the
    global path."""
    ep, eq = prob["edge_pose"], prob["edge_point"]
    e, _ = _residuals(quat_to_rot(poses[:, 3:])[ep], poses[ep, :3], points[eq], prob["meas"], prob["camera"])
    chi = prob["info"] * np.sum(e * e, axis=1)
    if not robust:
        return float(np.sum(chi)), chi
    delta = np.where(prob["meas"][:, 2] >= 0, delta_stereo, delta_mono)
    rho = np.where(chi <= delta * delta, chi, 2 * np.sqrt(chi) * delta - delta * delta)
    return float(np.sum(rho)), chi


def _se3_exp(u):
    """g2o's SE3Quat::exp of u = (omega, upsilon): R = exp([omega]x), t = V upsilon."""
    om, ups = np.asarray(u[:3], np.float64), np.asarray(u[3:], np.float64)
    th = float(np.linalg.norm(om))
    Om = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
    if th < 1e-5:
        a, b, c = 1.0, 0.5, 1.0 / 6.0
    else:
        a, b, c = np.sin(th) / th, (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    return np.eye(3) + a * Om + b * Om @ Om, (np.eye(3) + b * Om + c * Om @ Om) @ ups


def numpy_lm_first_step(prob, tau=1e-5, max_trials=10, h=1e-3):
    """One Levenberg-Marquardt iteration of the NON-robust problem, for small problems (dense H).  Returns (chi2 after the iteration,
    lambda after it, trials): what log[0] of a one-iteration, no-Huber solve holds.

    Independent of both implementations' analytic Jacobians: the residual Jacobian is a five-point central difference (step h) of
    _residuals, with the pose moved as g2o moves it - exp(omega, upsilon) applied on the LEFT - and the point additively.  Unknowns:
    the free poses that have an edge, then the points that have one.  H = J^T W J, b = -J^T W e, dense; lambda = tau * max diag H
    (computeLambdaInit, tau = 1e-5); (H + lambda I) x = b by numpy.linalg.solve; the step is judged as g2o does: rho =
    (chi2 - chi2_new) / (x . (lambda x + b) + 1e-3), accepted when positive, with lambda *= max(1/3, min(1 - (2 rho - 1)^3, 2/3)); else
    lambda *= nu, nu *= 2 and the step is tried again from the same estimate, max_trials times at most."""
    ep, eq, meas, cam, info = prob["edge_pose"], prob["edge_point"], prob["meas"], prob["camera"], prob["info"]
    E = len(ep)
    R0, t0, X0 = quat_to_rot(prob["poses"][:, 3:]), prob["poses"][:, :3].copy(), prob["points"].copy()
    free_poses = [k for k in range(len(t0)) if not prob["fixed"][k] and (ep == k).any()]
    seen_points = [p for p in range(len(X0)) if (eq == p).any()]
    pcol = {k: 6 * i for i, k in enumerate(free_poses)}
    xcol = {p: 6 * len(free_poses) + 3 * i for i, p in enumerate(seen_points)}
    n = 6 * len(free_poses) + 3 * len(seen_points)

    def res(Rm, t, X):
        return _residuals(Rm[ep], t[ep], X[eq], meas, cam)[0]

    def moved(Rm, t, u6):       # every pose moved by the same exp(u6), on the left
        Re, te = _se3_exp(u6)
        return Re @ Rm, t @ Re.T + te

    def diff(f):                # five-point central difference of f(step)
        return (8 * (f(h) - f(-h)) - (f(2 * h) - f(-2 * h))) / (12 * h)

    J = np.zeros((3 * E, n))
    rows = 3 * np.arange(E)
    for d in range(6):
        unit = np.eye(6)[d]
        col = diff(lambda s: res(*moved(R0, t0, s * unit), X0))         # [E, 3]: d e / d (pose of the edge)_d
        for e in range(E):
            if ep[e] in pcol:
                J[rows[e]:rows[e] + 3, pcol[ep[e]] + d] = col[e]
    for d in range(3):
        unit = np.eye(3)[d]
        col = diff(lambda s: res(R0, t0, X0 + s * unit))
        for e in range(E):
            J[rows[e]:rows[e] + 3, xcol[eq[e]] + d] = col[e]
    W = np.repeat(info, 3)
    e0 = res(R0, t0, X0).reshape(-1)
    chi = float(np.sum(W * e0 * e0))
    H = J.T @ (W[:, None] * J)
    b = -J.T @ (W * e0)
    lam, nu, trials = tau * float(np.max(np.diag(H))), 2.0, 0
    while True:
        x = np.linalg.solve(H + lam * np.eye(n), b)
        Rn, tn, Xn = R0.copy(), t0.copy(), X0.copy()
        for k in free_poses:
            Re, te = _se3_exp(x[pcol[k]:pcol[k] + 6])
            Rn[k], tn[k] = Re @ R0[k], Re @ t0[k] + te
        for p in seen_points:
            Xn[p] = X0[p] + x[xcol[p]:xcol[p] + 3]
        e1 = res(Rn, tn, Xn).reshape(-1)
        chi_new = float(np.sum(W * e1 * e1))
        rho = (chi - chi_new) / (float(x @ (lam * x + b)) + 1e-3)
        trials += 1
        if rho > 0 and np.isfinite(chi_new):
            lam *= max(1.0 / 3.0, min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0))
            chi = chi_new
            break
        lam *= nu
        nu *= 2
        if not (rho < 0 and trials < max_trials):
            break
    return chi, lam, trials


# numpy_lm_first_step against the oracle's log[0], relative: ten times the largest difference test_ba_structure_cpu.py measured
# (chi2 1.1e-13, lambda 1.6e-12)
LM_STEP_CHI2_RTOL = 1.1e-12
LM_STEP_LAMBDA_RTOL = 1.6e-11


# ---- rows of the structure tests: name -> builder; built once, read-only -----------------------------------------------------------
def _all_fixed(seed):
    return realistic_ba_problem(14, 500, seed, fixed=tuple(range(14)))


STRUCTURE_PROBLEMS = {
    "R1": lambda: realistic_ba_problem(seed=1),
    "R2": lambda: realistic_ba_problem(seed=2),
    # 0.1 rad / 0.1 m and 1.5 m from the truth: the one structure row on which the oracle rejects a step (in its third iteration)
    "R5-far": lambda: realistic_ba_problem(seed=5, pose_sigma=0.1, point_sigma=1.5),
    "back-fixed": lambda: with_backfacing_camera(realistic_ba_problem(seed=2), True),
    "back-free": lambda: with_backfacing_camera(realistic_ba_problem(seed=2), False),
    "one-free": lambda: realistic_ba_problem(2, 60, 1, fixed=(0,), n_unobserved=2, n_fixed_only=3, n_single=4),
    "all-fixed": lambda: _all_fixed(1),
    "small": lambda: realistic_ba_problem(5, 40, 1, fixed=(0,), n_unobserved=1, n_fixed_only=2, n_single=3),
    "small-mid": lambda: realistic_ba_problem(5, 40, 2, fixed=(2,), n_unobserved=1, n_fixed_only=2, n_single=3),
    "cap-2048": lambda: synth_ba_problem(3, 2048, 3, n_fixed=1),
    "cap-2049": lambda: synth_ba_problem(3, 2049, 3, n_fixed=1),
    "cap-2100": lambda: synth_ba_problem(3, 2100, 3, n_fixed=1),
}
GLOBAL6_R = ("global", 6, True)
GLOBAL6_N = ("global", 6, False)
GLOBAL1_N = ("global", 1, False)
BACKFACING_ROWS = ["back-fixed", "back-free"]
SMALL_ROWS = ["small", "small-mid"]
REALISTIC_ROWS = ["R1", "R2", "R5-far"] + BACKFACING_ROWS + ["one-free", "all-fixed"]    # realistic_ba_problem at its default noise model
CAP_ROWS = ["cap-2048", "cap-2049", "cap-2100"]                                          # 3 keyframes: diagonal pair buckets of P entries
# (id, problem, options) of every structure row that the GPU test compares with the oracle
STRUCTURE_ROWS = ([("%s-%s" % (n, t), n, s) for n in ("R1", "R2") for t, s in (("local", LOCAL), ("global-robust", GLOBAL6_R), ("global-plain", GLOBAL6_N))]
                  + [("%s-local" % n, n, LOCAL) for n in REALISTIC_ROWS[2:] + CAP_ROWS]
                  + [("%s-global1-plain" % n, n, GLOBAL1_N) for n in SMALL_ROWS])

