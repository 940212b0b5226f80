"""Restatement, without a GPU, of the occupancy score of pose hypotheses (include/wildcat_hip.h: wc_map_score_batch, wc_pose_grid,
wc_map_score_top).  It takes nothing from the library but an exported map - the voxels' keys and counts: the transform in
float64 numpy with the header's associations (numpy never fuses a multiply and an add), cast to float32; floor(q / v); the lookup in a
dict (score_ref) or in the sorted packed keys (score_fast: the same answer, vectorised for the 7056 poses of the scene); the pose grid in
longdouble and its bitwise forms; the ranking as a plain sorted().  Three deliberately wrong forms (drop_tile, float_P and the probe-chain
model with tomb_ends) show that the GPU test's inputs tell them from the right one."""
import numpy as np

import map_search_ref as MS
from extract_ref import LD

TILE = 256
KEY_LIM = 2**20
SCORE = np.dtype([("n_hit", np.uint32), ("n_in", np.uint32), ("n_bad", np.uint32), ("reserved", np.uint32)])
EMPTY, TOMB = 2**64 - 1, 2**64 - 2
MASK64 = 2**64 - 1

# the scene: DESIGN 8.10's room, scan and true pose, the start 9.9 m off, 16 headings x 21 x 21 x 1 positions at 0.8 m
SCENE_OFF = np.array([6.5, -7.5, 0.0])
SCENE_YAW, SCENE_N, SCENE_STEP = 16, (21, 21, 1), (0.8, 0.8, 0.0)
SCENE_TOP_M = 1
SCENE_ITERS = MS.SEARCH_ITERS


def scene_start():
    """(I | c + (6.5, -7.5, 0)) -> (3, 4)"""
    return np.concatenate([np.eye(3), (MS.SEARCH_C + SCENE_OFF)[:, None]], 1)


def moved(xyz, T, float_P=False):
    """q_a = (float)(((T[4a] x + T[4a+1] y) + T[4a+2] z) + T[4a+3]), x, y, z the floats cast to double -> (n, 3) float32.  float_P (a wrong
    form): the same expression in float32 arithmetic"""
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    T = np.asarray(T, np.float64).reshape(-1)[:12].reshape(3, 4)
    if float_P:
        with np.errstate(over="ignore"):
            T = T.astype(np.float32)
    else:
        p = p.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        P = np.stack([((T[a, 0] * p[:, 0] + T[a, 1] * p[:, 1]) + T[a, 2] * p[:, 2]) + T[a, 3] for a in range(3)], -1)
        return P.astype(np.float32)


def classify(xyz, T, v, float_P=False):
    """-> (k (n, 3) float64: floor((double)q / v), inside (n,) bool: the point counts in n_in, bad (n,) bool: it counts in n_bad)"""
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    q = moved(p, T, float_P)
    fin_p, fin_q = np.isfinite(p).all(1), np.isfinite(q).all(1)
    with np.errstate(invalid="ignore"):
        k = np.floor(q.astype(np.float64) / float(v))
        inside = fin_p & fin_q & (np.abs(k) < KEY_LIM).all(1)
    return k, inside, fin_p & ~fin_q


def _records(K):
    return np.zeros(K, SCORE)


def score_ref(keys, counts, v, xyz, Ts, min_points=1, drop_tile=None, float_P=False):
    """wc_map_score_batch on an exported map: keys (m, 3) integers, counts (m,) -> SCORE array (K,).  drop_tile (a wrong form): the points
    of that tile of 256 are left out"""
    table = {tuple(int(x) for x in k): int(c) for k, c in zip(np.asarray(keys).reshape(-1, 3), counts)}
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    keep = np.ones(len(p), bool)
    if drop_tile is not None:
        keep[drop_tile * TILE:(drop_tile + 1) * TILE] = False
    Ts = np.asarray(Ts, np.float64).reshape(len(Ts), -1)[:, :12]
    out = _records(len(Ts))
    for h, T in enumerate(Ts):
        k, inside, bad = classify(p, T, v, float_P)
        inside, bad = inside & keep, bad & keep
        out["n_in"][h], out["n_bad"][h] = inside.sum(), bad.sum()
        out["n_hit"][h] = sum(1 for kk in k[inside] if table.get((int(kk[0]), int(kk[1]), int(kk[2])), 0) >= min_points)
    return out


def pack(k):
    """the map's packed key: 21 bits per axis, offset 2^20 -> uint64"""
    k = np.asarray(k).astype(np.int64).reshape(-1, 3) + KEY_LIM
    return (k[:, 0].astype(np.uint64) << np.uint64(42)) | (k[:, 1].astype(np.uint64) << np.uint64(21)) | k[:, 2].astype(np.uint64)


def score_fast(keys, counts, v, xyz, Ts, min_points=1, float_P=False):
    """score_ref with the dict replaced by a search in the sorted packed keys of the voxels with count >= min_points"""
    live = np.sort(pack(np.asarray(keys).reshape(-1, 3)[np.asarray(counts).reshape(-1) >= min_points]))
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    Ts = np.asarray(Ts, np.float64).reshape(len(Ts), -1)[:, :12]
    out = _records(len(Ts))
    for h, T in enumerate(Ts):
        k, inside, bad = classify(p, T, v, float_P)
        out["n_in"][h], out["n_bad"][h] = inside.sum(), bad.sum()
        if len(live) and inside.any():
            pk = pack(k[inside])
            at = np.minimum(np.searchsorted(live, pk), len(live) - 1)
            out["n_hit"][h] = (live[at] == pk).sum()
    return out


# ---- the probe chain: a model of the table (splitmix64, linear probing, tombstones) for the wrong form that stops at a tombstone ----
def _hash(k):
    k ^= k >> 30
    k = (k * 0xBF58476D1CE4E5B9) & MASK64
    k ^= k >> 27
    k = (k * 0x94D049BB133111EB) & MASK64
    return k ^ (k >> 31)


def table_ref(keys, cap):
    """the packed keys inserted in the given order into `cap` slots (a power of two) -> list of slot words.  The device's slot order
    depends on its schedule; this is one of the tables it can build"""
    slots = [EMPTY] * cap
    for key in (int(x) for x in pack(keys)):
        h = _hash(key) & (cap - 1)
        while slots[h] != EMPTY:
            h = (h + 1) & (cap - 1)
        slots[h] = key
    return slots


def table_remove(slots, keys):
    gone = {int(x) for x in pack(keys)}
    return [TOMB if s in gone else s for s in slots]


def table_has(slots, key, tomb_ends=False):
    """the read-only probe chain: past foreign keys and tombstones up to the key or an empty slot.  tomb_ends (a wrong form): a
    tombstone ends the chain as an empty slot does"""
    cap = len(slots)
    h = _hash(key) & (cap - 1)
    for _ in range(cap):
        if slots[h] == key:
            return True
        if slots[h] == EMPTY or (tomb_ends and slots[h] == TOMB):
            return False
        h = (h + 1) & (cap - 1)
    return False


def score_table(slots, v, xyz, Ts, tomb_ends=False):
    """n_hit of score_ref (min_points 1) with the lookup made in a table_ref table -> (K,) counts"""
    out = np.zeros(len(Ts), np.uint32)
    for h, T in enumerate(np.asarray(Ts, np.float64).reshape(len(Ts), -1)[:, :12]):
        k, inside, _ = classify(xyz, T, v)
        out[h] = sum(1 for key in pack(k[inside]) if table_has(slots, int(key), tomb_ends))
    return out


# ---- wc_pose_grid -------------------------------------------------------------------------------------------------------------------
def grid_index(k, i, n):
    return ((k * n[0] + i[0]) * n[1] + i[1]) * n[2] + i[2]


def grid_offsets(n, step, dtype=np.float64):
    """per axis the offsets ((2 i - (n - 1)) 0.5) step_a, i < n_a, in `dtype`: the integer and the half are exact, the product is rounded"""
    return [(np.arange(int(na)) * 2 - (int(na) - 1)).astype(dtype) * dtype(0.5) * dtype(s) for na, s in zip(n, step)]


def pose_grid_bits(rot, T0, n, step):
    """the bitwise form: rot (n_yaw, 3, 4) the yaw grid of T0 (its rotations are taken as they are), translations
    t0_a + ((double)(2 i_a - (n_a - 1)) 0.5) step_a - one rounded product, one rounded sum -> (K, 3, 4) float64"""
    T0 = np.asarray(T0, np.float64).reshape(-1)[:12].reshape(3, 4)
    off = grid_offsets(n, step)
    out = np.zeros((len(rot) * n[0] * n[1] * n[2], 3, 4))
    for k in range(len(rot)):
        for i0 in range(n[0]):
            for i1 in range(n[1]):
                for i2 in range(n[2]):
                    T = out[grid_index(k, (i0, i1, i2), n)]
                    T[:, :3] = rot[k][:, :3]
                    T[:, 3] = [T0[0, 3] + off[0][i0], T0[1, 3] + off[1][i1], T0[2, 3] + off[2][i2]]
    return out


def pose_grid_ref(T0, n_yaw, n, step):
    """the grid in longdouble: MS.yaw_grid_ref's rotations, t0 + (i - (n - 1) / 2) step unrounded but for longdouble's own -> (K, 3, 4)"""
    rot = MS.yaw_grid_ref(T0, n_yaw)
    T0 = np.asarray(T0, np.float64).reshape(-1)[:12].reshape(3, 4).astype(LD)
    off = grid_offsets(n, step, LD)
    out = np.zeros((n_yaw * n[0] * n[1] * n[2], 3, 4), LD)
    for k in range(n_yaw):
        for i0 in range(n[0]):
            for i1 in range(n[1]):
                for i2 in range(n[2]):
                    T = out[grid_index(k, (i0, i1, i2), n)]
                    T[:] = rot[k]
                    T[:, 3] = [T0[0, 3] + off[0][i0], T0[1, 3] + off[1][i1], T0[2, 3] + off[2][i2]]
    return out


def top_ref(scores, M, min_hit):
    """wc_map_score_top: eligible iff n_bad == 0 and n_hit >= min_hit; larger n_hit first, then the smaller index -> (M indices, the rest
    -1; the count written)"""
    ok = sorted((h for h in range(len(scores)) if scores["n_bad"][h] == 0 and scores["n_hit"][h] >= min_hit),
                key=lambda h: (-int(scores["n_hit"][h]), h))[:M]
    return ok + [-1] * (M - len(ok)), len(ok)


# ---- the inputs of the GPU test (tests/test_map_score_gpu.py); tests/test_map_score_ref.py shows that the wrong forms change them -----
EQ_V, EQ_CLOUD, EQ_N, EQ_K = 0.5, 20_000, 8193, 1025
EQ_BAD, EQ_OUT = 7, 9  # the pose that sends every point to a non-finite one, and the one that sends every point out of the key range
# the pose and the point that tell float arithmetic from double: x = 2 - 0.3 u - 0.3 u, u = 2^-23 the float spacing below 2.  In double
# the sum is 2 - 0.6 u and rounds to the float 2 - u, voxel 3; in float each step rounds back to 2, voxel 4.  Voxel (3, 2, 2) of the
# map is empty and voxel (4, 2, 2) is not
EQ_FLOAT, EQ_FLOAT_POINT, EQ_FLOAT_AT = 11, (2.0, 1.0, 1.0), 1000


def eq_cloud():
    """the map's points: uniform over +-6 m -> (EQ_CLOUD, 3) float32; at v = 0.5 most voxels hold one to three points"""
    p = np.random.default_rng(21).uniform(-6.0, 6.0, (EQ_CLOUD, 3)).astype(np.float32)
    p[np.all(np.floor(p.astype(np.float64) / EQ_V) == (3, 2, 2), axis=1)] = (2.25, 1.25, 1.25)  # (EQ_FLOAT's two voxels)
    p[0] = (2.25, 1.25, 1.25)
    return p


def eq_scan():
    """EQ_N points: cloud points moved by 5 cm of noise, a quarter of them with a coordinate snapped onto a voxel face; a NaN and an inf"""
    rng = np.random.default_rng(22)
    p = eq_cloud()[rng.integers(0, EQ_CLOUD, EQ_N)].astype(np.float64) + rng.normal(size=(EQ_N, 3)) * 0.05
    snap = (rng.random((EQ_N, 3)) < 0.1) & (np.arange(EQ_N) % 4 == 0)[:, None]
    p = np.where(snap, np.rint(p / EQ_V) * EQ_V, p).astype(np.float32)
    p[5, 1], p[300, 0] = np.nan, np.inf
    p[EQ_FLOAT_AT] = EQ_FLOAT_POINT
    return p


def eq_poses():
    """EQ_K poses: identity, then rotations of a few degrees and translations of half a metre; EQ_BAD and EQ_OUT as named above"""
    import map_register_ref as G

    rng = np.random.default_rng(23)
    Ts = np.stack([np.concatenate([G.rodrigues(rng.normal(size=3) * 0.05), rng.normal(size=(3, 1)) * 0.5], 1) for _ in range(EQ_K)])
    Ts[0] = np.eye(3, 4)
    Ts[EQ_BAD] = np.concatenate([np.eye(3), np.full((3, 1), 1e39)], 1)
    Ts[EQ_OUT] = np.concatenate([np.eye(3), np.full((3, 1), 6e5)], 1)
    Ts[EQ_FLOAT] = np.eye(3, 4)
    Ts[EQ_FLOAT, 0, 1] = Ts[EQ_FLOAT, 0, 2] = -0.3 * 2.0**-23
    return Ts


def voxels_of(xyz, v):
    """the export of a map of these points, in numpy: (keys (m, 3) int64 in ascending order, counts (m,))"""
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    keys, counts = np.unique(np.floor(p / float(v)).astype(np.int64), axis=0, return_counts=True)
    return keys, counts


def flags(keys, counts, v, xyz, Ts, min_points=1):
    """score_fast before its sums: (hit, inside, bad), each (K, n) bool - the records of every prefix of the points come from one pass"""
    live = np.sort(pack(np.asarray(keys).reshape(-1, 3)[np.asarray(counts).reshape(-1) >= min_points]))
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    Ts = np.asarray(Ts, np.float64).reshape(len(Ts), -1)[:, :12]
    hit, ins, bad = (np.zeros((len(Ts), len(p)), bool) for _ in range(3))
    for h, T in enumerate(Ts):
        k, ins[h], bad[h] = classify(p, T, v)
        if len(live) and ins[h].any():
            pk = pack(k[ins[h]])
            at = np.minimum(np.searchsorted(live, pk), len(live) - 1)
            hit[h, ins[h]] = live[at] == pk
    return hit, ins, bad


def records_of(fl, n, K):
    """the SCORE records of the first n points and the first K poses of flags()'s arrays"""
    out = _records(K)
    out["n_hit"], out["n_in"], out["n_bad"] = (f[:K, :n].sum(1) for f in fl)
    return out


# the crowded table: CROWD_M voxels in a table of 2 CROWD_M slots (reserve_voxels = CROWD_M: the fullest a table gets), every third removed
CROWD_V, CROWD_M = 0.5, 2048


def crowd_keys():
    """CROWD_M distinct voxel indices within +-20 -> (CROWD_M, 3) int32"""
    rng = np.random.default_rng(24)
    flat = rng.permutation(41**3)[:CROWD_M]
    return (np.stack([flat // 1681, (flat // 41) % 41, flat % 41], 1) - 20).astype(np.int32)


def centres(keys, v):
    """the voxels' centres (dyadic for v = 0.5: exact in float32) -> (m, 3) float32"""
    return ((np.asarray(keys, np.float64) + 0.5) * v).astype(np.float32)


def crowd_poses():
    """identity and shifts by one voxel along each axis"""
    Ts = np.tile(np.eye(3, 4), (4, 1, 1))
    for a in range(3):
        Ts[a + 1, a, 3] = CROWD_V
    return Ts
