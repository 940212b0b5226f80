"""Restatement, without a GPU, of the search over pose hypotheses (include/wildcat_hip.h: wc_map_align_best, wc_pose_yaw_grid,
wc_map_align_pyramid_batch): the winner's rule in plain Python, the yaw grid in longdouble, and the search as a loop of
map_register_ref.align over hypotheses and levels; and the scene of DESIGN 8.10 - the room of 8.9 seen from an unknown heading."""
from fractions import Fraction

import numpy as np

import map_coarsen_ref as MC
import map_register_ref as G
from extract_ref import LD
from helpers import xyz_of as _xyz
from wildcat_slam_amd import synth

PI = LD("3.14159265358979323846264338327950288")
WC_OK = 0

# the scene: the room of 8.9 as the map (levels 1.6 -> 0.2), a 4000-point scan taken 100 degrees of yaw and 3 of roll away from the start
# (I | c), K = 8 yaw hypotheses, 10 iterations per level
SEARCH_C = np.array([2.0, -1.0, 1.5])
SEARCH_K, SEARCH_ITERS, SEARCH_SCAN = 8, 10, 4000


def rot_z(a):
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


def rot_x(a):
    return np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]])


def search_pose():
    """the true pose (Rz(100 deg) Rx(3 deg) | c + (0.3, -0.2, 0.1)) -> (3, 4)"""
    return np.concatenate([rot_z(np.deg2rad(100.0)) @ rot_x(np.deg2rad(3.0)), (SEARCH_C + np.array([0.3, -0.2, 0.1]))[:, None]], 1)


def search_start():
    """(I | c) -> (3, 4)"""
    return np.concatenate([np.eye(3), SEARCH_C[:, None]], 1)


def search_scan():
    """g1_room(4000, seed + 7) taken into the sensor frame of the true pose, as float32: R^T (p - t)"""
    T = search_pose()
    p = _xyz(synth.g1_room(SEARCH_SCAN, seed=synth.SEED + 7)).astype(np.float64)
    return ((p - T[:, 3]) @ T[:, :3]).astype(np.float32)


def search_sizes():
    """the levels' voxel sizes, coarsest first"""
    return MC.basin_sizes()[::-1]


def best_ref(summaries, status, min_used):
    """wc_map_align_best: eligible iff status 0, termination != 2, n_used >= min_used and a finite final_cost; most n_used first, then the
    smaller final_cost, then the smaller index -> index or -1"""
    ok = [h for h, (s, st) in enumerate(zip(summaries, status))
          if st == WC_OK and s["termination"] != 2 and s["n_used"] >= min_used and np.isfinite(s["final_cost"])]
    return min(ok, key=lambda h: (-summaries[h]["n_used"], summaries[h]["final_cost"], h)) if ok else -1


def yaw_grid_ref(T0, K):
    """(Rz(2 pi k / K) R0 | t0), k < K, in longdouble -> (K, 3, 4).  The turn k / K is split exactly into quarter turns and a rest below
    one (Fractions), so sine and cosine are taken of an angle below pi / 2 and carry longdouble's rounding alone"""
    T0 = np.asarray(T0, np.float64).reshape(-1)[:12].reshape(3, 4).astype(LD)
    out = np.zeros((K, 3, 4), LD)
    for k in range(K):
        turn = Fraction(k, K)
        quarter = int(turn * 4)
        rest = turn - Fraction(quarter, 4)
        a = (LD(2) * PI * LD(rest.numerator)) / LD(rest.denominator)
        c, s = np.cos(a), np.sin(a)
        for _ in range(quarter):  # (a quarter turn more: (c, s) -> (-s, c))
            c, s = -s, c
        out[k] = T0
        out[k, 0, :3] = c * T0[0, :3] - s * T0[1, :3]
        out[k, 1, :3] = s * T0[0, :3] + c * T0[1, :3]
    return out


def search_ref(surfels_of, scan, Ts, sizes, params_of, iters=SEARCH_ITERS):
    """every start of Ts through the levels of voxel sizes `sizes`, in that order, each by map_register_ref.align from the pose the level
    before it left.  surfels_of(v): the MAP_SURFEL records of the level of voxel size v; params_of(v): its registration parameters
    -> (Ts (K, 3, 4), [[summary per hypothesis] per level])"""
    Ts = np.array(Ts, np.float64).reshape(-1, 3, 4)
    summ = [[None] * len(Ts) for _ in sizes]
    for h in range(len(Ts)):
        for l, v in enumerate(sizes):
            Ts[h], summ[l][h] = G.align(surfels_of(v), scan, Ts[h], v, params_of(v), max_iterations=iters, tol_rot=G.TOL_ROT, tol_trans=G.TOL_TRANS)
    return Ts, summ


def report(Ts, finest, T_true):
    """the table of DESIGN 8.10: per hypothesis (n_used, final_cost, termination, rotation error [rad], translation error [m])"""
    return [(s["n_used"], s["final_cost"], s["termination"]) + G.pose_error(T, T_true) for T, s in zip(Ts, finest)]
