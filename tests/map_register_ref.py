"""Restatement, without a GPU, of the registration against the voxel map (include/wildcat_hip.h: wc_map_linearize, wc_map_align) on an
exported map - PointMap.surfels(), or surfels_cpu() below, map_surfel_ref's planes as MAP_SURFEL records: the rows in numpy float64 with
the header's associations (numpy never fuses a multiply and an add: meant to be bit-exact), the sums in longdouble with compensated
summation, the number of additions A(n), and the Gauss-Newton loop in float64."""
import numpy as np

import map_query_ref as Q
import map_surfel_ref as S
from extract_ref import LD
from wildcat_slam_amd import records as R

EPS = 2.0**-53
TILE, FAN = 256, 32
# the recovery test (v = 0.8f, no loss): scan size and the loop's tolerances.  The restatement's steps fall 7e-5, 1e-5, 7e-9 m and
# 2e-5, 4e-7, 8e-10 rad and then stay at the 1e-9 level the float rounding of the moved points leaves: the step that meets these
# tolerances is more than 10 x under them (test_map_register_ref.py checks it)
N_ALIGN, TOL_ROT, TOL_TRANS = 20_000, 1e-7, 1e-6
# H's upper triangle, row-major: entry e = (a, b)
UPPER = [(a, b) for a in range(6) for b in range(a, 6)]


def surfels_cpu(xyz, v):
    """the MAP_SURFEL records of a moments map of the points xyz, from map_surfel_ref alone: exact integer sums, the correctly rounded
    covariance, eigenpairs by the longdouble Jacobi iteration rounded to float64.  (A map on the device differs from it by a few ulps of
    the eigen-solve; the restatement below only needs planes, whichever solver made them.)"""
    sums = S.voxel_sums(xyz, v)
    m = len(sums["count"])
    out = np.zeros(m, R.MAP_SURFEL)
    out["key"], out["count"] = sums["keys"], sums["count"]
    c = sums["count"].astype(np.float64)[:, None]
    out["xyz"] = (S.map_ref(sums["keys"], v) + sums["Q"].astype(np.float64) / (c * S.UNIT_Q)).astype(np.float32)
    for i in range(m):
        n = int(sums["count"][i])
        out["cov"][i] = [N / (n * n * 2**32) for N in S.numerators(n, sums["U"][i], sums["M"][i])]
    ev, nrm = S.eigen_ref(out["cov"])
    out["ev"], out["normal"] = ev.astype(np.float64), nrm.astype(np.float64)
    out["flags"] = ((out["count"] >= 3) & (out["ev"][:, 2] > 0)).astype(np.uint32)
    return out


def transform(xyz, T):
    """q_a = (float)(((T[4a] x + T[4a+1] y) + T[4a+2] z) + T[4a+3]) with x, y, z the floats cast to double -> (n, 3) float32"""
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    T = np.asarray(T, np.float64).reshape(-1)[:12].reshape(3, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        P = np.stack([((T[a, 0] * p[:, 0] + T[a, 1] * p[:, 1]) + T[a, 2] * p[:, 2]) + T[a, 3] for a in range(3)], -1)
        return P.astype(np.float32)


def rows_ex(surf, xyz, T, v, params):
    """wc_map_linearize's per-point part -> dict(rows: MAP_REG_ROW array, rho, w2 (float64, 0 where unused), used (bool), n_used,
    n_found, hits: the MAP_PLANE_HIT records of the moved points).  params: anything with max_dist, min_points, sigma0, cauchy_a"""
    q = transform(xyz, T)
    hits, _ = S.plane_hits(surf, q, v, params.max_dist, params.min_points)
    used = (hits["flags"] & 2) != 0
    Qd = q.astype(np.float64)
    n, d = hits["normal"], hits["dist"]
    s02, a2 = float(params.sigma0) * float(params.sigma0), float(params.cauchy_a) * float(params.cauchy_a)
    out = np.zeros(len(q), R.MAP_REG_ROW)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        J = np.stack([Qd[:, 1] * n[:, 2] - Qd[:, 2] * n[:, 1], Qd[:, 2] * n[:, 0] - Qd[:, 0] * n[:, 2], Qd[:, 0] * n[:, 1] - Qd[:, 1] * n[:, 0],
                      n[:, 0], n[:, 1], n[:, 2]], -1)
        w2 = 1.0 / (s02 + hits["sigma2"])
        s = (w2 * d) * d
        if a2 > 0.0:
            u = s / a2
            k, rho = w2 / (1.0 + u), a2 * np.log1p(u)
        else:
            k, rho = w2, s
    out["J"] = np.where(used[:, None], J, 0.0)
    out["d"] = np.where(used, d, 0.0)
    out["k"] = np.where(used, k, 0.0)
    return dict(rows=out, rho=np.where(used, rho, 0.0), w2=np.where(used, w2, 0.0), used=used, n_used=int(used.sum()),
                n_found=int((hits["count"] != 0).sum()), hits=hits)


def rows(surf, xyz, T, v, params):
    """-> the MAP_REG_ROW array alone"""
    return rows_ex(surf, xyz, T, v, params)["rows"]


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def comp_sum(x):
    """sum of the longdouble array x by pairwise halving with every addition's error carried along (error-free transformations): far
    below the longdouble rounding of a single addition for the lengths used here"""
    x = np.asarray(x, LD).reshape(-1)
    if len(x) == 0:
        return LD(0)
    err = np.zeros_like(x)
    while len(x) > 1:
        if len(x) % 2:
            x, err = np.append(x, LD(0)), np.append(err, LD(0))
        s, e = _two_sum(x[0::2], x[1::2])
        x, err = s, err[0::2] + err[1::2] + e
    return x[0] + err[0]


def normal_eq(rows, w2=None, cauchy_a=0.0):
    """the sums of the rows' doubles in longdouble -> dict(H (21,), g (6,), absH (21,), absg (6,): sum |term| per entry, cost, abscost:
    sum |rho| / 2).  A term is the exact product k J_a J_b (k J_a d) of the doubles - three 53-bit factors do not fit longdouble's 64 bits,
    so it carries one longdouble rounding per product, 2^-11 of a double's.  cost needs the weights w2 of rows_ex: s = w2 d d and
    rho = a^2 log1p(s / a^2) with longdouble's log1p (rho = s without a loss)."""
    J, d, k = rows["J"].astype(LD), rows["d"].astype(LD), rows["k"].astype(LD)
    H, absH = np.zeros(21, LD), np.zeros(21, LD)
    for e, (a, b) in enumerate(UPPER):
        t = (k * J[:, a]) * J[:, b]
        H[e], absH[e] = comp_sum(t), comp_sum(np.abs(t))
    g, absg = np.zeros(6, LD), np.zeros(6, LD)
    for a in range(6):
        t = (k * J[:, a]) * d
        g[a], absg[a] = comp_sum(t), comp_sum(np.abs(t))
    out = dict(H=H, g=g, absH=absH, absg=absg)
    if w2 is not None:
        s = (np.asarray(w2).astype(LD) * d) * d
        a2 = LD(float(cauchy_a) * float(cauchy_a))
        rho = a2 * np.log1p(s / a2) if a2 > 0 else s
        out["cost"] = out["abscost"] = LD(0.5) * comp_sum(rho)  # (rho >= 0)
    return out


def adds_bound(n):
    """A(n): the largest number of floating-point additions a term passes through (include/wildcat_hip.h: wc_map_linearize)"""
    if n <= 0:
        return 0
    adds, m = (FAN - 1) + (TILE // FAN - 1), -(-n // TILE)
    while m > 1:
        adds += min(FAN, m) - 1
        m = -(-m // FAN)
    return adds


def device_order_sum(terms, dtype=np.float64, drop_tile=None):
    """the sum of the per-point terms in the order the header states (tiles of 256, chunks of 32, levels of 32), in `dtype`; drop_tile:
    that tile's partial is left out (what a broken second stage would do)"""
    t = np.asarray(terms, dtype)
    n = len(t)
    if n == 0:
        return dtype(0)
    t = np.concatenate([t, np.zeros(-n % TILE, dtype)]).reshape(-1, TILE // FAN, FAN)
    chunk = t[:, :, 0].copy()
    for j in range(1, FAN):
        chunk = (chunk + t[:, :, j]).astype(dtype)
    part = chunk[:, 0].copy()
    for c in range(1, TILE // FAN):
        part = (part + chunk[:, c]).astype(dtype)
    if drop_tile is not None:
        part[drop_tile] = 0
    while len(part) > 1:
        m = len(part)
        p = np.concatenate([part, np.zeros(-m % FAN, dtype)]).reshape(-1, FAN)
        real = np.concatenate([np.ones(m, bool), np.zeros(-m % FAN, bool)]).reshape(-1, FAN)
        acc = p[:, 0].copy()
        for j in range(1, FAN):  # (a short last group adds nothing beyond its own partials)
            acc = np.where(real[:, j], (acc + p[:, j]).astype(dtype), acc)
        part = acc
    return part[0]


def full(H21):
    """(21,) upper triangle -> (6, 6) symmetric"""
    A = np.zeros((6, 6), np.asarray(H21).dtype)
    for e, (a, b) in enumerate(UPPER):
        A[a, b] = A[b, a] = H21[e]
    return A


def rodrigues(w):
    """Rod(w) = I + A K + B K^2, A = sin(th) / th, B = (sin(th/2) / (th/2))^2 / 2, as csrc/map.hip forms it"""
    wx, wy, wz = (float(x) for x in w)
    th = np.sqrt((wx * wx + wy * wy) + wz * wz)
    A, B = 1.0, 0.5
    if th > 0.0:
        h = np.sin(0.5 * th) / (0.5 * th)
        A, B = np.sin(th) / th, 0.5 * (h * h)
    K = np.array([[0.0, -wz, wy], [wz, 0.0, -wx], [-wy, wx, 0.0]])
    E = np.zeros((3, 3))
    for r in range(3):
        for c in range(3):
            k2 = (K[r, 0] * K[0, c] + K[r, 1] * K[1, c]) + K[r, 2] * K[2, c]
            E[r, c] = ((1.0 if r == c else 0.0) + A * K[r, c]) + B * k2
    return E


def pose_update(T, xi):
    """R <- Rod(omega) R, t <- Rod(omega) t + upsilon -> (3, 4)"""
    T = np.asarray(T, np.float64).reshape(-1)[:12].reshape(3, 4)
    E = rodrigues(xi[:3])
    N = np.zeros((3, 4))
    for r in range(3):
        for c in range(4):
            N[r, c] = ((E[r, 0] * T[0, c] + E[r, 1] * T[1, c]) + E[r, 2] * T[2, c]) + (float(xi[3 + r]) if c == 3 else 0.0)
    return N


def gn_step(H21, g, min_pivot):
    """H xi = -g by Cholesky of H scaled to unit diagonal, float64 -> (xi or None, pivots): None when a pivot is not finite or < min_pivot"""
    A = full(np.asarray(H21, np.float64))
    g = np.asarray(g, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        D = 1.0 / np.sqrt(np.diag(A))
    L, piv = np.zeros((6, 6)), []
    for i in range(6):
        for j in range(i + 1):
            with np.errstate(invalid="ignore"):
                s = 1.0 if i == j else (D[i] * A[i, j]) * D[j]
            for k in range(j):
                s -= L[i, k] * L[j, k]
            if i == j:
                piv.append(s)
                if not (np.isfinite(s) and np.isfinite(D[i]) and s >= min_pivot):
                    return None, piv
                L[i, i] = np.sqrt(s)
            else:
                L[i, j] = s / L[j, j]
    y, xi = np.zeros(6), np.zeros(6)
    for i in range(6):
        s = -(D[i] * g[i])
        for k in range(i):
            s -= L[i, k] * y[k]
        y[i] = s / L[i, i]
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s -= L[k, i] * xi[k]
        xi[i] = s / L[i, i]
    xi = xi * D
    return (xi if np.all(np.isfinite(xi)) else None), piv


def linearize(surf, xyz, T, v, params):
    """wc_map_linearize restated: the rows, then the sums in float64 in the device's order -> (H (21,), g (6,), cost, n_used, n_found)"""
    r = rows_ex(surf, xyz, T, v, params)
    J, d, k = r["rows"]["J"], r["rows"]["d"], r["rows"]["k"]
    H = np.array([device_order_sum((k * J[:, a]) * J[:, b]) for a, b in UPPER])
    g = np.array([device_order_sum((k * J[:, a]) * d) for a in range(6)])
    return H, g, 0.5 * float(device_order_sum(r["rho"])), r["n_used"], r["n_found"]


def align(surf, xyz, T, v, params, max_iterations=20, tol_rot=1e-6, tol_trans=1e-6, min_used=6, min_pivot=1e-9):
    """wc_map_align restated in float64 -> (T (3, 4), dict as wc_map_align_summary)"""
    T = np.asarray(T, np.float64).reshape(-1)[:12].reshape(3, 4).copy()
    out = dict(initial_cost=0.0, final_cost=0.0, iterations=0, termination=1, n_used=0, n_found=0, last_step=np.zeros(6))
    fresh, lin = False, None
    for it in range(max_iterations):
        lin = linearize(surf, xyz, T, v, params)
        fresh = True
        if it == 0:
            out["initial_cost"] = lin[2]
        xi = gn_step(lin[0], lin[1], min_pivot)[0] if lin[3] >= min_used else None
        if xi is None:
            out["termination"] = 2
            break
        T = pose_update(T, xi)
        fresh = False
        out["last_step"], out["iterations"] = xi, it + 1
        if np.linalg.norm(xi[:3]) <= tol_rot and np.linalg.norm(xi[3:]) <= tol_trans:
            out["termination"] = 0
            break
    if not fresh:
        lin = linearize(surf, xyz, T, v, params)
    out["final_cost"], out["n_used"], out["n_found"] = lin[2], lin[3], lin[4]
    return T, out


def pose_error(T, T_true):
    """-> (rotation angle [rad] of R R_true^T, |t - t_true| [m])"""
    T, T_true = np.asarray(T, np.float64).reshape(3, 4), np.asarray(T_true, np.float64).reshape(3, 4)
    dR = T[:, :3] @ T_true[:, :3].T
    w = 0.5 * np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])
    return float(np.arctan2(np.linalg.norm(w), 0.5 * (np.trace(dR) - 1.0))), float(np.linalg.norm(T[:, 3] - T_true[:, 3]))


# ---- the hand map (v = 0.5): three faces of a corner, every coordinate dyadic on the 2^-16 m grid --------------------------------------
# Face x = 0.125 is sampled in the voxels (0, j, k), face y = 0.125 in (i, 0, k), face z = 0.125 in (i, j, 0), i, j, k in {1, 2}: four
# voxels per face, each with the same 3 x 3 grid of points (offsets 0.125, 0.25, 0.375 inside the voxel), so every covariance is diagonal
# with an exactly zero row across the face: ev[0] = 0 and the normal is exactly the face's axis.
HAND_V = 0.5
HAND_FACE = 0.125


def hand_corner():
    """-> (points (108, 3) float32, axis (108,): which face a point lies on)"""
    pts, axis = [], []
    off = (0.125, 0.25, 0.375)
    for ax in range(3):
        o1, o2 = [a for a in range(3) if a != ax]
        for i in (1, 2):
            for j in (1, 2):
                for u in off:
                    for w in off:
                        p = [0.0, 0.0, 0.0]
                        p[ax], p[o1], p[o2] = HAND_FACE, i * HAND_V + u, j * HAND_V + w
                        pts.append(p)
                        axis.append(ax)
    return np.array(pts, np.float32), np.array(axis)


def hand_wall():
    """a single plane: the face z = 0.125 alone -> (36, 3) float32"""
    p, ax = hand_corner()
    return p[ax == 2]
