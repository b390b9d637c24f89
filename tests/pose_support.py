"""Shared case table for the pose-only optimiser (Optimizer::optimizePose, optimizer.cpp:358-501): named problems in
ydorbslam_amd.synth.synth_pose_problem's format, one per branch of k_pose_optimize (ydorbslam_amd/csrc/ba_kernels.hip.h) and of its
oracle yo_pose_optimize (oracle/ba_oracle.cpp).  tests/test_pose_cpu.py proves on the oracle's per-episode trace that every case
reaches the branch it is here for; tests/test_pose_gpu.py runs the same table through the kernel.

Also here: an independent numpy statement of the cost that both minimise, written from the formulae of g2o's
types_six_dof_expmap.h (EdgeSE3ProjectXYZOnlyPose / EdgeStereoSE3ProjectXYZOnlyPose::computeError) and not from the oracle's code,
and the tolerance that goes with it."""
import numpy as np

from ydorbslam_amd.synth import synth_pose_problem

EDGE_KEYS = ("points", "meas", "info", "is_gross_outlier")
TH_MONO, TH_STEREO = np.float32(5.991), np.float32(7.815)      # optimizer.cpp:467,484, compared in float
CUT_COUNTS = (0, 1, 2, 3, 9, 10, 11, 63, 64, 65, 255, 256, 257, 513)


def cut(prob, n):
    """The first n correspondences of prob (same start pose, same camera)."""
    return {k: (np.ascontiguousarray(v[:n]) if k in EDGE_KEYS else v) for k, v in prob.items()}


def empty_frame(like):
    """A frame without any correspondence, with `like`'s pose and camera."""
    return cut(like, 0)


def qnormalized(pose):
    """The start pose as both sides hold it: the quaternion divided by its norm (two roundings: the square root and the quotient)."""
    p = np.asarray(pose, np.float64).copy()
    p[3:] = p[3:] / np.sqrt(p[3] * p[3] + p[4] * p[4] + p[5] * p[5] + p[6] * p[6])
    return p


# ---- the independent reference ------------------------------------------------------------------------------------------------
def edge_chi2(prob, pose, dtype=np.float64):
    """info_e |z_e - pi(R X_e + t)|^2 of every edge at `pose` (tx, ty, tz, qx, qy, qz, qw), no robust kernel:
    types_six_dof_expmap.h: cam_project is (fx x/z + cx, fy y/z + cy), the stereo edge adds u - bf/z; R is the unit quaternion as a
    rotation matrix.  Every operation in `dtype`."""
    f = lambda a: np.asarray(a, dtype)
    t, (x, y, z, w) = f(pose[:3]), f(pose[3:])
    one, two = dtype(1), dtype(2)
    Rm = np.array([[one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)],
                   [two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)],
                   [two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)]], dtype)
    X, m, info = f(prob["points"]).reshape(-1, 3), f(prob["meas"]).reshape(-1, 3), f(prob["info"])
    fx, fy, cx, cy, bf = f(prob["camera"])
    # R X + t row by row in elementwise operations (one rounding each on any machine; a BLAS product may fuse or reorder them)
    xc, yc, zc = (Rm[i, 0] * X[:, 0] + Rm[i, 1] * X[:, 1] + Rm[i, 2] * X[:, 2] + t[i] for i in range(3))
    u = fx * xc / zc + cx
    v = fy * yc / zc + cy
    stereo = m[:, 2] >= 0
    du, dv = m[:, 0] - u, m[:, 1] - v
    dr = np.where(stereo, m[:, 2] - (u - bf / zc), dtype(0))
    return info * (du * du + dv * dv + dr * dr)


def reprojection_cost(prob, pose, dtype=np.float64):
    """sum_e edge_chi2: the cost that optimizePose minimises once no robust kernel is left, over every edge."""
    return edge_chi2(prob, pose, dtype).sum(dtype=dtype)


def cost_and_bound(prob, pose):
    """(cost in float64, cost in longdouble, bound).  The difference of the two evaluations is what one ordering of float64 roundings
    costs on these inputs; the oracle and the kernel order the rotation (quaternion sandwich, not a matrix) and the sum (edge order /
    256 strided lanes and a wave butterfly, not numpy's pairwise sum) differently, each such difference about as large as the one
    measured, hence 16 times it."""
    c64 = reprojection_cost(prob, pose, np.float64)
    cld = reprojection_cost(prob, pose, np.longdouble)
    return float(c64), cld, 16.0 * abs(float(np.longdouble(c64) - cld))


def _rotation(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def quiet(prob, scale=0.25):
    """prob with its measurement noise shrunk: z <- pi(truth) + scale * (z - pi(truth)), rounded to float again.  synth_pose_problem's
    1-sigma pixel noise puts 5 % of clean edges past the chi2 thresholds; the all-inlier cases need every edge to stay inside in
    every episode (scale 0.25: chi2 / 16)."""
    tp = prob["truth_pose"]
    Xc = prob["points"] @ _rotation(tp[3:]).T + tp[:3]
    fx, fy, cx, cy, bf = prob["camera"]
    u, v = fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy
    exact = np.stack([u, v, u - bf / Xc[:, 2]], axis=1)
    m = prob["meas"].copy()
    st = m[:, 2] >= 0
    m[:, :2] = exact[:, :2] + scale * (m[:, :2] - exact[:, :2])
    m[st, 2] = exact[st, 2] + scale * (m[st, 2] - exact[st, 2])
    out = dict(prob)
    out["meas"] = m.astype(np.float32).astype(np.float64)
    return out


# ---- the table ----------------------------------------------------------------------------------------------------------------
def _build():
    T = {}
    base = synth_pose_problem(600, seed=16, outlier_frac=0.1)
    for n in CUT_COUNTS:
        T["cut_%d" % n] = cut(base, n)
    T["all_mono"] = synth_pose_problem(40, seed=21, mono_frac=1.0)
    T["all_stereo"] = synth_pose_problem(40, seed=23, mono_frac=0.0)          # (a seed whose right coordinates are all >= 0)
    z = synth_pose_problem(400, seed=23)
    z["info"] = np.zeros_like(z["info"])
    T["zero_info"] = z
    na = synth_pose_problem(400, seed=24)
    noise = np.random.default_rng(2400).normal(0, 200, (400, 3))
    m = na["meas"].copy()
    st = m[:, 2] >= 0
    m[:, :2] += noise[:, :2]
    m[st, 2] = np.abs(m[st, 2] + noise[st, 2])               # a stereo edge stays one (ur >= 0)
    na["meas"] = m.astype(np.float32).astype(np.float64)
    T["no_active_edge"] = na
    T["far_start_06"] = synth_pose_problem(300, seed=9, pose_noise=0.6)
    T["far_start_03"] = synth_pose_problem(300, seed=9, pose_noise=0.3)
    T["near_start_002"] = synth_pose_problem(300, seed=9, pose_noise=0.02)
    T["late_exclusion"] = synth_pose_problem(200, seed=382, outlier_frac=0.3, pose_noise=0.05)
    uz = synth_pose_problem(40, seed=23, mono_frac=0.0)
    tp, (fx, fy, cx, cy, bf) = uz["truth_pose"], uz["camera"]
    depth, u, v = 5.0, bf / 5.0 + 0.8, 250.0                 # edge 0: at the image's left edge the right coordinate is 0.8 px ...
    Xc = np.array([(u - cx) * depth / fx, (v - cy) * depth / fy, depth])
    for k in ("points", "meas", "info"):
        uz[k] = uz[k].copy()
    uz["points"][0] = (_rotation(tp[3:]).T @ (Xc - tp[:3])).astype(np.float32)
    uz["meas"][0] = np.array([u, v, 0.0], np.float32)        # ... and measured as exactly 0.0: still a stereo edge (ur >= 0)
    uz["info"][0] = 1.0
    T["right_coordinate_zero"] = uz
    one = synth_pose_problem(1, seed=25, outlier_frac=0.0, mono_frac=0.0)
    T["rank_deficient"] = {k: (np.repeat(v, 12, axis=0) if k in EDGE_KEYS else v) for k, v in one.items()}
    nn = synth_pose_problem(400, seed=26)
    nn["points"] = nn["points"].copy()
    nn["points"][137] = np.nan
    T["nan_point"] = nn
    T["inliers_mono_40"] = quiet(synth_pose_problem(40, seed=27, outlier_frac=0.0, mono_frac=1.0))
    T["inliers_stereo_40"] = quiet(synth_pose_problem(40, seed=26, outlier_frac=0.0, mono_frac=0.0))
    T["inliers_mixed_300"] = quiet(synth_pose_problem(300, seed=29, outlier_frac=0.0, mono_frac=0.3))
    return T


CASES = _build()

# What each case is in the table for.  test_pose_cpu.py asserts every one of these statements on the oracle.
PURPOSE = {
    "cut_0": "E = 0: nothing to do, 0 returned, pose untouched",
    "cut_1": "E < 3 exit (:443-445): 0 returned, pose untouched",
    "cut_2": "E < 3 exit, largest such E",
    "cut_3": "smallest E that optimises; E < 10: one episode only (:494)",
    "cut_9": "E < 10 exit: one finite chi2, three NaN",
    "cut_10": "first E with four episodes: four finite chi2",
    "cut_11": "four episodes",
    "cut_63": "stride loops: one edge short of a wave",
    "cut_64": "stride loops: one wave exactly",
    "cut_65": "stride loops: one wave and one edge",
    "cut_255": "stride loops: one pass of the 256 threads, one lane idle",
    "cut_256": "stride loops: one full pass",
    "cut_257": "stride loops: one pass and one edge",
    "cut_513": "stride loops: two passes and one edge",
    "all_mono": "every edge two-dimensional (J row 2 zero, threshold 5.991)",
    "all_stereo": "every edge three-dimensional (threshold 7.815)",
    "zero_info": "H + lambda I = 0: every dense_solve<6> fails, the (zero) step is still applied; 40 trials, pose returned as given",
    "no_active_edge": "every edge excluded after episode 0: nAct == 0 in episodes 1-3, which log NaN",
    "far_start_06": "episode 0 spends its ten iterations far from the optimum, every edge is excluded: nAct == 0 afterwards",
    "far_start_03": "the same draw from 0.3 converges to the inlier set of the 0.02 start",
    "near_start_002": "the reference inlier set of the seed-9 draw",
    "late_exclusion": "an edge that episode 3 optimised over ends beyond its threshold: chi2[3] is a plain sum, not a Huber sum",
    "right_coordinate_zero": "ur == 0.0 exactly is a stereo edge (the test is ur >= 0, `ur < 0` -> mono)",
    "rank_deficient": "twelve copies of one edge: rank-3 H, the lambda I term alone keeps Cholesky going",
    "nan_point": "non-finite input: NaN chi2 in every episode; the oracle leaves through !isfinite(lambda), the kernel's fmax drops the NaN",
    "inliers_mono_40": "no flag ever set: chi2[3] is the plain cost over every edge",
    "inliers_stereo_40": "no flag ever set, stereo",
    "inliers_mixed_300": "no flag ever set, two passes of the stride loop",
}
ALL_INLIER = ("inliers_mono_40", "inliers_stereo_40", "inliers_mixed_300")
BELOW_THREE = ("cut_0", "cut_1", "cut_2")
# where the LM trial count cannot depend on rounding: (case, trials)
FIXED_TRIALS = {"cut_0": 0, "cut_1": 0, "cut_2": 0, "zero_info": 40, "no_active_edge": 10, "far_start_06": 10}
# where the optimum is an exact fit: the logged chi2 is rounding residue (1e-21 against start costs of 1e3), not comparable at rtol 1e-6
CHI2_AT_ROUNDING_FLOOR = ("rank_deficient",)
# where the oracle hands back the start pose (normalised)
START_POSE_RETURNED = ("zero_info", "no_active_edge", "far_start_06", "nan_point")


def batch_order():
    """The whole table as one batch, a zero-edge frame after every case: (names, problems), name None for the fillers."""
    names, probs = [], []
    for k in CASES:
        names += [k, None]
        probs += [CASES[k], empty_frame(CASES[k])]
    return names, probs
