"""numpy restatements of the voxel map's query and crop (include/wildcat_hip.h: wc_map_nearest, wc_map_crop), on an exported map:
keys (n, 3) int32 in ascending (kx, ky, kz) order, centroids (n, 3) float32, counts (n,) uint32 - what PointMap.export() or
test_map_cpu.downsample_voxel return."""
import itertools

import numpy as np

from wildcat_slam_amd import records as R

KEY_LIM = 2**20


def pack(k):
    """(n, 3) voxel indices -> the packed 63-bit key: ascending packed key = ascending (kx, ky, kz)"""
    k = np.asarray(k, np.int64).reshape(-1, 3)
    return ((k[:, 0] + KEY_LIM) << 42) | ((k[:, 1] + KEY_LIM) << 21) | (k[:, 2] + KEY_LIM)


def dist2(q64, c32):
    """(dx*dx + dy*dy) + dz*dz in float64, dx = (double)q.x - (double)c.x"""
    d = q64 - np.asarray(c32, np.float32).astype(np.float64)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def search(keys, cen, q, v):
    """the search of wc_map_nearest before max_dist is applied -> (ok: the query could be searched, best d2 or inf, row or -1).
    The 27 offsets are visited in ascending key order and a later one wins only with a strictly smaller d2: ties go to the smaller key."""
    q64 = np.asarray(q, np.float32).reshape(-1, 3).astype(np.float64)
    n = len(q64)
    packed = pack(np.asarray(keys).reshape(-1, 3))
    assert np.all(packed[1:] > packed[:-1]), "the export is in ascending key order"
    cen = np.asarray(cen, np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        kf = np.floor(q64 / v)
        ok = np.all(np.isfinite(kf) & (kf > -float(KEY_LIM)) & (kf < float(KEY_LIM)), axis=1)
    kq = np.where(ok[:, None], kf, 0.0).astype(np.int64)
    best = np.full(n, np.inf)
    idx = np.full(n, -1, np.int64)
    if len(packed):
        for off in itertools.product((-1, 0, 1), repeat=3):  # ascending (kx, ky, kz)
            nk = kq + np.array(off, np.int64)
            inside = ok & np.all((nk > -KEY_LIM) & (nk < KEY_LIM), axis=1)
            pk = pack(np.where(inside[:, None], nk, 0))
            pos = np.minimum(np.searchsorted(packed, pk), len(packed) - 1)
            occ = inside & (packed[pos] == pk)
            with np.errstate(invalid="ignore", over="ignore"):
                d2 = dist2(q64, cen[pos])
            better = occ & (d2 < best)
            best = np.where(better, d2, best)
            idx = np.where(better, pos, idx)
    return ok, best, idx


def accept(keys, cen, cnt, found, max_dist):
    """the answer records of a search(): a candidate is accepted iff d2 <= max_dist * max_dist -> (hits: R.MAP_HIT array, row or -1)"""
    ok, best, idx = found
    md2 = float(max_dist) * float(max_dist)
    hit = (idx >= 0) & (best <= md2)
    idx = np.where(hit, idx, -1)
    hits = np.zeros(len(ok), R.MAP_HIT)
    hits["flags"] = np.where(ok, 0, 1)
    hits["d2"] = np.where(hit, best, np.inf)
    if len(np.asarray(cnt)):
        at = np.maximum(idx, 0)
        hits["xyz"] = np.where(hit[:, None], np.asarray(cen, np.float32).reshape(-1, 3)[at], np.float32(0))
        hits["count"] = np.where(hit, np.asarray(cnt, np.uint32)[at], 0)
        hits["key"] = np.where(hit[:, None], np.asarray(keys, np.int32).reshape(-1, 3)[at], 0)
    return hits, idx


def nearest_voxel(keys, cen, cnt, q, v, max_dist):
    """wc_map_nearest restated on an exported map -> (hits: R.MAP_HIT array, idx: row of the export that was hit, -1 for none)"""
    return accept(keys, cen, cnt, search(keys, cen, q, v), max_dist)


def brute_force(cen, q, max_dist, chunk=256):
    """the globally nearest centroid within max_dist, every centroid tried -> (idx or -1, d2 or inf); the first (smallest key) of
    equal distances wins"""
    q64 = np.asarray(q, np.float32).reshape(-1, 3).astype(np.float64)
    cen = np.asarray(cen, np.float32).reshape(-1, 3)
    idx, best = np.full(len(q64), -1, np.int64), np.full(len(q64), np.inf)
    for s in range(0, len(q64), chunk):
        d2 = dist2(q64[s : s + chunk, None, :], cen[None, :, :])
        j = np.argmin(d2, axis=1)
        idx[s : s + chunk], best[s : s + chunk] = j, d2[np.arange(len(j)), j]
    hit = best <= float(max_dist) * float(max_dist)
    return np.where(hit, idx, -1), np.where(hit, best, np.inf)


def crop_keep(keys, v, lo, hi):
    """wc_map_crop's keep mask: floor(lo[a] / v) <= k[a] <= floor(hi[a] / v) on every axis"""
    k = np.asarray(keys).reshape(-1, 3).astype(np.float64)
    klo, khi = np.floor(np.asarray(lo, np.float64) / v), np.floor(np.asarray(hi, np.float64) / v)
    return np.all((k >= klo) & (k <= khi), axis=1)


def point_keys(xyz, v):
    """VoxelLoc of every point, as float64 (NaN / inf stay what they are)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.floor(np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64) / v)


def pow2_at_least(x):
    c = 1
    while c < x:
        c <<= 1
    return c


# ---- the hand-worked case (v = 0.5, dyadic coordinates, voxel counts 1 and 2: every centroid is exact in any arithmetic) ----------
HAND_V = 0.5
HAND_POINTS = np.array(
    [
        [0.25, 0.25, 0.25],  # A: voxel (0, 0, 0)
        [0.75, 0.25, 0.25],  # B: voxel (1, 0, 0)
        [1.625, 0.125, 0.125],  # C: voxel (3, 0, 0), two points, centroid (1.75, 0.25, 0.25)
        [1.875, 0.375, 0.375],
        [-0.25, -0.25, -0.25],  # D: voxel (-1, -1, -1)
    ],
    np.float32,
)
HAND_KEYS = [[-1, -1, -1], [0, 0, 0], [1, 0, 0], [3, 0, 0]]  # export order: D, A, B, C
HAND_CENTROIDS = [[-0.25, -0.25, -0.25], [0.25, 0.25, 0.25], [0.75, 0.25, 0.25], [1.75, 0.25, 0.25]]
HAND_COUNTS = [1, 1, 1, 2]
HAND_QUERIES = np.array(
    [
        [0.5, 0.25, 0.25],  # 0: on the face between A and B (own voxel (1, 0, 0)), 0.25 from both: the smaller key, A, wins
        [0.0, 0.25, 0.25],  # 1: on the face x = 0 (own voxel (0, 0, 0)): A at 0.25; D at d2 = 0.5625
        [1.375, 0.25, 0.25],  # 2: own voxel (2, 0, 0) is empty; B at d2 = 0.390625, C at 0.140625
        [0.25, 0.25, 0.5],  # 3: A at exactly 0.25: accepted with max_dist = 0.25
        [3.25, 0.25, 0.25],  # 4: voxel (6, 0, 0), two voxels and more from anything: a miss whatever max_dist
        [-0.125, -0.125, -0.125],  # 5: negative coordinates: D at d2 = 3 / 64
        [np.nan, 0, 0],  # 6 - 9: cannot be searched
        [0, np.inf, 0],
        [2.0**19, 0, 0],  # voxel 2^20
        [-(2.0**19) - 0.5, 0, 0],  # voxel -2^20 - 1
        [2.0**19 - 0.25, 0, 0],  # 10: voxel 2^20 - 1, the last one inside the range (its +1 neighbours are skipped): a plain miss
    ],
    np.float32,
)
# per max_dist: (row of the export hit or -1, d2) per query
HAND_EXPECT = {
    np.inf: ([1, 1, 3, 1, -1, 0, -1, -1, -1, -1, -1], [0.0625, 0.0625, 0.140625, 0.0625, np.inf, 0.046875] + [np.inf] * 5),
    0.25: ([1, 1, -1, 1, -1, 0, -1, -1, -1, -1, -1], [0.0625, 0.0625, np.inf, 0.0625, np.inf, 0.046875] + [np.inf] * 5),
    float(np.nextafter(0.25, 0)): ([-1, -1, -1, -1, -1, 0, -1, -1, -1, -1, -1], [np.inf] * 5 + [0.046875] + [np.inf] * 5),
}
HAND_FLAGS = [0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0]


def hand_expected_hits(max_dist):
    idx, d2 = HAND_EXPECT[max_dist]
    hits = np.zeros(len(idx), R.MAP_HIT)
    for i, j in enumerate(idx):
        if j >= 0:
            hits["xyz"][i], hits["count"][i], hits["key"][i] = HAND_CENTROIDS[j], HAND_COUNTS[j], HAND_KEYS[j]
    hits["d2"], hits["flags"] = d2, HAND_FLAGS
    return hits, np.array(idx)
