"""Restatement, without a GPU, of the voxel map's coarser levels (include/wildcat_hip.h: wc_map_coarsen): every fine voxel's
integer sums re-based to the coarse voxel's reference point with Python integers wrapped to 64 bits, then added up by coarse key with
map_state_ref.absorb_ref; and the mask of the points whose coarse voxel, found from the fine one, is not the one a direct insert finds."""
import numpy as np

import map_state_ref as MS
import map_surfel_ref as S
from wildcat_slam_amd import records as R

MASK64 = 2**64 - 1


def _wrap(x):
    return ((x + 2**63) & MASK64) - 2**63


def coarse_voxel(v, factor):
    """V = (double)factor * v: one fp64 product"""
    return float(factor) * float(v)


def shifts(keys, v, factor):
    """-> (K (n, 3) int64: floor(k / factor), D (n, 3) Python ints: (r(k, v) - r(K, V)) 2^32, a multiple of 2^22)"""
    k = np.asarray(keys, np.int64).reshape(-1, 3)
    K = k // int(factor)  # (numpy's // rounds toward minus infinity)
    d = (S.map_ref(k, v) - S.map_ref(K, coarse_voxel(v, factor))) * S.UNIT_Q
    assert np.all(d == np.rint(d)) and np.all(np.abs(d) < 2.0**62)
    D = [[int(x) for x in row] for row in d]
    assert all(x % 2**22 == 0 for row in D for x in row)
    return K, D


def rebase(vox, mom, v, factor):
    """the records of a state, each re-based to its coarse voxel (key K; the keys are no longer distinct) -> (vox, mom or None)"""
    K, D = shifts(vox["key"], v, factor)
    out = np.zeros(len(vox), R.MAP_VOXEL)
    out["key"], out["count"] = K, vox["count"]
    out_mom = None if mom is None else np.zeros((len(vox), 9), np.int64)
    for i in range(len(vox)):
        n = int(vox["count"][i])
        d = D[i]
        e = [x >> 16 for x in d]
        out["sum"][i] = [_wrap(int(vox["sum"][i][a]) + n * d[a]) for a in range(3)]
        if mom is not None:
            U = [int(x) for x in mom[i][:3]]
            M = [int(x) for x in mom[i][3:]]
            out_mom[i][:3] = [_wrap(U[a] + n * e[a]) for a in range(3)]
            out_mom[i][3:] = [_wrap(M[j] + e[a] * U[b] + e[b] * U[a] + n * e[a] * e[b]) for j, (a, b) in enumerate(S.PAIRS)]
    return out, out_mom


def coarsen_ref(vox, mom, v, factor):
    """wc_map_coarsen restated on a state -> (vox, mom or None) of the map of voxel size (double)factor * v; mom None: a plain result"""
    rv, rm = rebase(vox, mom, v, factor)
    out, out_mom, n_rej = MS.absorb_ref([(rv, rm)], moments=mom is not None)
    assert n_rej == 0
    return out, out_mom


def face_cloud(n, v, factor, seed, span=6.0, share=0.4):
    """(n, 3) float32 over +-span m, negative coordinates included; `share` of the points have one or more coordinates snapped onto a
    face of the fine grid (float32(j v)), half of those onto a face of the coarse grid (float32(j factor v))"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-span, span, (n, 3))
    m = int(share * n)
    for lo, hi, step in ((0, m // 2, float(v)), (m // 2, m, coarse_voxel(v, factor))):
        snap = rng.random((hi - lo, 3)) < 0.5
        snap[np.arange(hi - lo), rng.integers(0, 3, hi - lo)] = True  # (at least one axis)
        p[lo:hi] = np.where(snap, np.rint(p[lo:hi] / step) * step, p[lo:hi])
    return p.astype(np.float32)


# the basin case: a 60 000-point room as the map at v = 0.2, a 4000-point scan 12 degrees and 0.8 m off, levels 1.6 -> 0.2
BASIN_V, BASIN_FACTOR, BASIN_LEVELS, BASIN_ROOM, BASIN_SCAN, BASIN_ITERS = 0.2, 2, 4, 60_000, 4000, 30


def basin_pose():
    """12 degrees about (0.3, -0.4, 0.866) / |.| and 0.8 (0.6, -0.64, 0.48) m -> (3, 4)"""
    import map_register_ref as G

    axis = np.array([0.3, -0.4, 0.866])
    axis /= np.linalg.norm(axis)
    return np.concatenate([G.rodrigues(np.deg2rad(12.0) * axis), (0.8 * np.array([0.6, -0.64, 0.48]))[:, None]], 1)


def basin_sizes():
    """the levels' voxel sizes, finest first: each (double)factor times the one before"""
    vs = [BASIN_V]
    for _ in range(1, BASIN_LEVELS):
        vs.append(coarse_voxel(vs[-1], BASIN_FACTOR))
    return vs


def basin_ref(surfels_of, scan, params_of, sizes):
    """the float64 restatement from identity through the levels of voxel sizes `sizes`, in that order.  surfels_of(v): the MAP_SURFEL
    records of the level of voxel size v; params_of(v): its registration parameters -> (T, [summary per level])"""
    import map_register_ref as G

    T, summ = np.eye(3, 4), []
    for v in sizes:
        T, s = G.align(surfels_of(v), scan, T, v, params_of(v), max_iterations=BASIN_ITERS, tol_rot=G.TOL_ROT, tol_trans=G.TOL_TRANS)
        summ.append(s)
    return T, summ


def disagree(xyz, v, factor):
    """the points p with floor((double)p / V) != floor(floor((double)p / v) / factor) on an axis: a direct insert at V puts them into
    another coarse voxel than the coarsening of their fine voxel does"""
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    direct = np.floor(p / coarse_voxel(v, factor))
    via = np.floor(p / v).astype(np.int64) // int(factor)
    return np.any(direct.astype(np.int64) != via, axis=1)
