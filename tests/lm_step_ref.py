"""One damped Levenberg-Marquardt step of the window solve, restated in float64 numpy, and the tools that judge a computed step.

The step as Ceres takes it (oracle/window.cc: the solve's ComputeStep; csrc/window.hip: damped_entry and lm_step), with all
n = 12 ns unknowns kept - the rows the gauge zeroes come out as a zero step:
    scale = 1 / (1 + sqrt(diag H)),  Hs = S H S,  gs = S g
    D = clip(diag Hs, 1e-6, 1e32),  A = Hs + diag(D) / radius
    y = A^-1 gs,  step = -S y
The residual A y - gs is formed by Dot2 (Ogita, Rump and Oishi, "Accurate sum and dot product", SISC 2005): every product split
exactly by Dekker's algorithm, every sum by Knuth's TwoSum - as accurate as a dot product in twice the working precision, then
rounded once, in plain float64 on any machine (no long double)."""
import numpy as np

_SPLITTER = 134217729.0  # 2^27 + 1: Dekker's split of a double into two 26-bit halves


def _split(a):
    c = _SPLITTER * a
    hi = c - (c - a)
    return hi, a - hi


def two_prod(a, b):
    """p + e == a * b exactly (Dekker / Veltkamp; no FMA needed)"""
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, al * bl - (((p - ah * bh) - al * bh) - ah * bl)


def two_sum(a, b):
    """s + e == a + b exactly (Knuth)"""
    s = a + b
    z = s - a
    return s, (a - (s - z)) + (b - z)


def dot2_residual(A, y, b):
    """r = A y - b row by row by Dot2: |r - exact| <= eps |exact| + O(eps^2) * sum |A_ij y_j| + |b_i|"""
    A = np.asarray(A, np.float64)
    y = np.asarray(y, np.float64)
    At = np.ascontiguousarray(A.T)
    p = -np.asarray(b, np.float64).copy()
    s = np.zeros_like(p)
    for j in range(len(y)):
        h, r = two_prod(At[j], y[j])
        p, q = two_sum(p, h)
        s += q + r
    return p + s


def damped_system(H, g, radius, scale=None):
    """(A, gs, scale) of the damped, Jacobi-scaled system one LM step solves; scale: that of the solve's FIRST linearisation, which
    Ceres keeps for every later one (None: H is the first)"""
    H = np.asarray(H, np.float64)
    if scale is None:
        scale = 1.0 / (1.0 + np.sqrt(np.diag(H)))
    A = H * scale[:, None] * scale[None, :]
    gs = np.asarray(g, np.float64) * scale
    D = np.clip(np.diag(A), 1e-6, 1e32)
    A[np.diag_indices_from(A)] += D / radius
    return A, gs, scale


def solve(A, b, refine=3):
    """A^-1 b by numpy's Cholesky, then `refine` steps of iterative refinement on the Dot2 residual"""
    L = np.linalg.cholesky(A)

    def chol(r):
        return np.linalg.solve(L.T, np.linalg.solve(L, r))

    y = chol(b)
    for _ in range(refine):
        y = y - chol(dot2_residual(A, y, b))
    return y


def reference_step(H, g, radius=1e4, refine=3):
    """the step (= the solve's first increment at x) of the damped system built from H and g"""
    A, gs, scale = damped_system(H, g, radius)
    return -scale * solve(A, gs, refine)


def backward_errors(A, gs, y, rows=None):
    """normwise backward error eta = ||A y - gs||_inf / (||A||_inf ||y||_inf + ||gs||_inf) of a computed y; `rows` (name -> index
    array): the same measure restricted to those rows, each with its own block's norms (an error confined to small rows is not
    hidden by the large ones)"""
    r = dot2_residual(A, y, gs)
    arow = np.abs(A).sum(axis=1)
    ynorm = np.abs(y).max()
    out = {}
    for name, idx in (("all", slice(None)),) + tuple((rows or {}).items()):
        den = arow[idx].max() * ynorm + np.abs(gs[idx]).max()
        out[name] = float(np.abs(r[idx]).max() / den) if den > 0 else 0.0
    return out


def pose_bias_rows(ns):
    """row indices of the pose (local 0..5) and bias (local 6..11) unknowns of every sample state"""
    k = np.arange(12 * ns)
    return {"pose": np.nonzero(k % 12 < 6)[0], "bias": np.nonzero(k % 12 >= 6)[0]}


# ---- the synthetic windows the step is tested on (CPU only: synth + the oracle's matcher) ----------------------------------------
FAMILIES = ("default", "free_gauge", "no_imu", "one_plane", "weak_imu")
WEAK_IMU = 1e-6  # weak_imu: every IMU weight times this - the bias unknowns' diag(S H S) falls below the LM clamp (1e-6)


def window_shape(ns):
    """(n_scans, patches per scan, sample_dt) of a synthetic window with exactly ns sample states: synth.surfel_window makes
    floor(n_scans * 0.5 / sample_dt) + 2 of them, and sample_dt sits half a state away from the floor's steps"""
    n_scans = max(2, -(-ns // 34))
    return n_scans, max(150, 16 * ns // n_scans), n_scans * 0.5 / (ns - 1.5)


def _rotate_inv(quat, v):
    """R(quat)^T v for arrays of unit quaternions (w, x, y, z)"""
    w_, u = quat[:, 0:1], -quat[:, 1:4]
    t = 2.0 * np.cross(u, v)
    return v + w_ * t + np.cross(u, t)


def window_problem(oracle, ns, family="default", seed=11, max_iterations=1):
    """a window of ns sample states of one family: default (gauge held, IMU factors), free_gauge (fix_first_pos = 0: the gauge is
    held by the IMU factors alone), no_imu (the bias block is damping only), one_plane (every surfel normal is the world z axis:
    two translations and yaw unobservable by lidar), weak_imu (IMU weights scaled by WEAK_IMU).  Correspondences by the oracle."""
    from wildcat_slam_amd import synth

    assert family in FAMILIES
    n_scans, patches, dt = window_shape(ns)
    w = synth.surfel_window(n_scans, patches, seed=seed, fixed_patches=patches // 3, sample_dt=dt)
    assert len(w["sample_times"]) == ns
    if family == "one_plane":
        for k_s, k_p in (("surf", "pose"), ("fix_surf", "fix_pose")):
            w[k_s]["normal"] = _rotate_inv(w[k_p]["quat"], np.tile(np.array([[0.0, 0.0, 1.0]]), (len(w[k_s]), 1)))
    params = oracle.default_params()
    params.max_iterations = max_iterations
    if family == "weak_imu":
        for k in ("w_gyr", "w_acc", "w_bg", "w_ba"):
            setattr(params, k, getattr(params, k) * WEAK_IMU)
    pairs = oracle.match(w["surf"], w["pose"], w["surf"], w["pose"], True, params)
    pf = oracle.match(w["surf"], w["pose"], w["fix_surf"], w["fix_pose"], False, params)
    return dict(w=w, params=params, pairs=pairs, pf=pf, fix_first=family != "free_gauge", imu=None if family == "no_imu" else w["imu"])


def oracle_window(oracle, prob):
    w = prob["w"]
    W = oracle.Window(w["sample_times"], w["grav"], prob["fix_first"], prob["params"])
    W.add_binary(w["surf"], w["pose"], prob["pairs"])
    W.add_unary(w["fix_surf"], w["fix_pose"], w["surf"], w["pose"], prob["pf"])
    if prob["imu"] is not None:
        W.add_imu(prob["imu"])
    return W

