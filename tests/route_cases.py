"""The planted inputs of tests/test_route_edges_gpu.py: clouds whose owner sequence is prescribed, clouds with points on the voxel
rule's edges, crafted surfel lists for the k-way merge and the small clouds of the sharded call.  Everything here is built with
tests/route_ref.py alone; tests/test_route_ref.py asserts without a GPU that every case is what its name claims."""
import numpy as np

import route_ref as RR
from wildcat_slam_amd import records as R
from wildcat_slam_amd import synth

V_DEFAULT = np.float32(0.8)  # wc_params_default
NS = (1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097, 6143)  # ends inside a wavefront, a 256-lane iteration, a 2048-point tile
WORLDS = (1, 2, 3, 7, 8, 63, 64)
N_MAX = 6143
SEQ_WORLDS = (2, 3, 8, 64)
SEQ_BOUNDS = (64, 256, 2048)  # a wavefront, an iteration, a tile of k_route_scatter
F32 = np.float32


def make_points(xyz, t=None):
    """POINT records with strictly ascending stamps (so that a partition that is not stable shows) and junk in the fields the
    partition must not read"""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    n = len(xyz)
    pts = np.zeros(n, R.POINT)
    pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pts["time"] = 100.0 + 0.001 * np.arange(n) if t is None else t
    pts["intensity"] = np.arange(n) % 251
    pts["ring"] = (7 * np.arange(n)) % 65521
    return pts


def random_cloud(n, seed=1):
    rng = np.random.default_rng(seed)
    return make_points(rng.uniform(-20, 20, size=(n, 3)))


def expected(points, segs):
    """the records wc_route_partition must write for the segments of partition_ref -> (ROUTE_POINT array, counts)"""
    idx = np.concatenate(segs).astype(np.int64) if len(segs) else np.zeros(0, np.int64)
    out = np.zeros(len(idx), R.ROUTE_POINT)
    for f, h in (("x", "x"), ("y", "y"), ("z", "z"), ("t", "time")):
        out[f] = points[h][idx]
    return out, [len(s) for s in segs]


# ---- prescribed owner sequences ------------------------------------------------------------------------------------------
def seq_one(n, world):
    return np.full(n, world - 1, np.int64)


def seq_cycle(n, world):
    return np.arange(n, dtype=np.int64) % world


def seq_steps(n, world):
    return np.searchsorted(np.array(SEQ_BOUNDS), np.arange(n), side="right").astype(np.int64) % world


def seq_random(n, world):
    return np.random.default_rng(7 + world).integers(0, world, n).astype(np.int64)


SEQS = {"one": seq_one, "cycle": seq_cycle, "steps": seq_steps, "random": seq_random}


def owner_cloud(world, seq, voxel=V_DEFAULT):
    """a cloud whose point i lies at the centre of a voxel that rank seq[i] owns"""
    keys = RR.keys_owned_by(world)
    centres = ((keys + 0.5) * np.float64(F32(voxel))).astype(F32)
    return make_points(centres[np.asarray(seq, np.int64)])


# ---- the voxel rule's edges ----------------------------------------------------------------------------------------------------
FACE_KS = (-100000, -1001, -37, -3, -2, -1, 0, 1, 2, 3, 37, 1001, 100000)


def face_values(voxel):
    """per k of FACE_KS: (the float below float32(k v), float32(k v), the float above)"""
    v = np.float64(F32(voxel))
    out = []
    for k in FACE_KS:
        f = F32(k * v)
        out.append((np.nextafter(f, F32(-np.inf)), f, np.nextafter(f, F32(np.inf))))
    return out


def edge_values(voxel):
    """coordinates on the voxel rule's edges: faces and their float neighbours, zeros and subnormals, quotients next to and beyond the
    int32 range, non-finite values"""
    v = np.float64(F32(voxel))
    vals = [x for tri in face_values(voxel) for x in tri]
    vals += [F32(-0.0), F32(0.0), F32(1e-45), F32(-1e-45), F32(1e-39), F32(-1e-39), F32(1.17549435e-38), F32(-1.17549435e-38)]
    for q in (2147483648.0, 2147483647.0, -2147483648.0, -2147483649.0):
        f = F32(q * v)
        vals += [np.nextafter(f, F32(-np.inf)), f, np.nextafter(f, F32(np.inf))]
    vals += [F32(3e9 * v), F32(-3e9 * v), np.finfo(F32).max, -np.finfo(F32).max]
    vals += [F32(np.nan), F32(np.inf), F32(-np.inf)]
    return np.array(vals, F32)


def edge_cloud(voxel, n_random=1500, seed=3):
    """every value of edge_values on every axis in turn (the two other coordinates ordinary), a few points with three special
    coordinates, all mixed into a random cloud at random places"""
    rng = np.random.default_rng(seed)
    vals = edge_values(voxel)
    rows = []
    for axis in range(3):
        xyz = rng.uniform(-20, 20, size=(len(vals), 3)).astype(F32)
        xyz[:, axis] = vals
        rows.append(xyz)
    big = F32(-3e9 * np.float64(F32(voxel)))
    rows.append(np.array([[np.nan, np.nan, np.nan], [np.inf, -np.inf, np.nan], [big, big, big], [-0.0, -0.0, -0.0], [1e-45, -1e-45, 0.0]], F32))
    rows.append(rng.uniform(-20, 20, size=(n_random, 3)).astype(F32))
    xyz = np.concatenate(rows)
    return make_points(xyz[rng.permutation(len(xyz))])


# ---- crafted surfel lists for the merge ------------------------------------------------------------------------------------------
def _surfels(j, ts):
    """list j's records: only t steers the merge, center carries (list, position), the rest is filler that must travel along"""
    n = len(ts)
    p = np.arange(n, dtype=np.float64)
    s = np.zeros(n, R.SURFEL)
    s["t"] = ts
    s["center"][:, 0], s["center"][:, 1], s["center"][:, 2] = j, p, -1.5
    s["cov"] = (1000.0 * j + p)[:, None] + np.arange(9)[None, :] / 16.0
    s["normal"] = np.array([0.0, 0.6, -0.8])[None, :] * (1.0 + p[:, None])
    s["resolution"] = 0.4
    s["sigma"] = j + p / 4096.0
    return s


def _ids(rows):
    i = np.zeros(len(rows), R.SURFEL_ID)
    for f, c in zip(("kx", "ky", "kz", "node"), range(4)):
        i[f] = [r[c] for r in rows]
    return i


def _from_rows(per_list):
    """per list the rows (t, kx, ky, kz, node), in the list's order -> (lists, id_lists)"""
    lists = [_surfels(j, np.array([r[0] for r in rows], np.float64)) for j, rows in enumerate(per_list)]
    return lists, [_ids([r[1:] for r in rows]) for rows in per_list]


def canon(row):
    return (row[0], row[1], row[2], row[3], row[4] & RR.M32)


def _deal(pool, assign, k):
    per = [[] for _ in range(k)]
    for row, j in zip(sorted(pool, key=canon), assign):
        per[int(j)].append(row)
    return per


def _pool(rng, n, n_t, n_id):
    """n rows with stamps from n_t values and ids from n_id values: ties of every kind"""
    idv = [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(rng.integers(-3, 3, n_id), rng.integers(-3, 3, n_id), rng.integers(-3, 3, n_id), rng.integers(0, 9, n_id))]
    return [(float(rng.integers(0, n_t)) / 8.0,) + idv[int(rng.integers(0, n_id))] for _ in range(n)]


BIG_LIST = 17
_MERGE = {}


def merge_cases():
    """name -> dict(lists, ids): every list sorted by (t, kx, ky, kz, node as unsigned), as the merge expects"""
    if _MERGE:
        return _MERGE
    rng = np.random.default_rng(11)

    def put(name, per_list, with_ids=True):
        lists, ids = _from_rows(per_list)
        _MERGE[name] = dict(lists=lists, ids=ids if with_ids else None, rows=per_list)

    put("k1", _deal(_pool(rng, 300, 50, 40), np.zeros(300, int), 1))
    # 64 lists of 0 - 3 records, few stamps and ids: ties across many lists
    counts = rng.integers(0, 4, 64)
    counts[0], counts[5], counts[63] = 3, 0, 3
    put("k64_small", _deal(_pool(rng, int(counts.sum()), 6, 3), rng.permutation(np.repeat(np.arange(64), counts)), 64))
    # empty lists first, last and adjacent
    put("empties", _deal(_pool(rng, 77, 12, 5), rng.permutation(np.repeat(np.arange(7), (0, 0, 40, 0, 0, 37, 0))), 7))
    # one list of 1 000 records (distinct stamps) and 63 singletons: equal to a record of the long list (lists in front of it and
    # behind it), between two of its records, in front of all and behind all
    big = [(0.5 * p, p % 5 - 2, -(p % 3), p % 7, p % 11) for p in range(1000)]
    per = []
    for j in range(64):
        if j == BIG_LIST:
            per.append(big)
        elif j % 4 == 0:
            per.append([big[(37 * j) % 1000]])
        elif j % 4 == 1:
            per.append([(big[(53 * j) % 1000][0] + 0.25, 0, 0, 0, 0)])
        elif j % 4 == 2:
            per.append([big[(53 * j) % 1000][:4] + (big[(53 * j) % 1000][4] + 1,)])  # the stamp and voxel of a record, the next node id
        else:
            per.append([(-1.0 if j < 32 else 1e4, 0, 0, 0, 0)])
    put("big_and_singletons", per)
    for n in (255, 256, 257):
        put("total_%d" % n, _deal(_pool(rng, n, 30, 20), rng.integers(0, 3, n), 3))
    # list 1 wholly behind list 0, list 2 wholly in front of both
    put("front_behind", [[(10.0 + p / 128.0, p % 3, 0, 0, p) for p in range(100)], [(20.0 + p / 128.0, 0, p % 3, 0, p) for p in range(100)],
                         [(p / 128.0, 0, 0, p % 3, p) for p in range(100)]])
    # every stamp equal: the ids alone order the records - negative indices, node ids on both sides of 2^31
    ks = (RR.INT32_MIN, -2, -1, 0, 1, RR.INT32_MAX)
    nodes = (0, 1, 5, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFF)
    pool = set()
    while len(pool) < 400:
        pool.add((5.0, ks[rng.integers(0, 6)], ks[rng.integers(0, 6)] if rng.random() < 0.5 else 0, int(rng.integers(-1, 2)), nodes[rng.integers(0, 7)]))
    pool = sorted(pool, key=canon)
    put("equal_stamps", _deal(pool, rng.integers(0, 5, len(pool)), 5))
    # the same (t, id) in 64, 3 and 2 lists, and twice in one list
    a, b, c, d = (1.0, -4, 2, 0, 7), (2.0, 3, -1, 5, 0x80000000), (3.0, 0, 0, -9, 1), (4.0, 1, 1, 1, 1)
    per = []
    for j in range(64):
        rows = [a]
        if j in (3, 7, 20):
            rows.append(b)
        if j in (3, 7):
            rows.append(c)
        if j == 7:
            rows += [d, d]
        if j == 9:
            rows.append(d)
        rows.append((5.0 + j, j, 0, 0, 0))
        per.append(rows)
    put("dups", per)
    # no ids at all: only the stamps compare, ties in list order
    put("no_ids", _deal(_pool(rng, 500, 25, 4), rng.integers(0, 6, 500), 6), with_ids=False)
    return _MERGE


# ---- the sharded search: (queries, ranks, k) ---------------------------------------------------------------------------------------
MATCH_SHARD_FROM, MATCH_MAX_WORLD, MATCH_GROUP = 4096, 8, 8  # csrc/match.hip: shards from 4 096 queries, at most 8 ranks, 8 queries a wavefront
MATCH_CASES = [(4095, 3, 10), (4096, 3, 10), (4099, 3, 10), (4099, 5, 10), (4099, 7, 10), (4099, 8, 10), (4104, 8, 10), (4099, 5, 3), (4099, 5, 16)]


def match_shares(nq, world):
    """the positions [begin, end) of the query order every rank searches"""
    return [((nq * r) // world, (nq * (r + 1)) // world) for r in range(world)]


# ---- the sharded call's small clouds -------------------------------------------------------------------------------------------
LATTICE_SEED = 4


def one_root_cloud():
    """256 points in ONE root voxel"""
    return synth.g2_lattice(1, m=32, seed=3)


def lattice12():
    """twelve root voxels, 3 072 points"""
    return synth.g2_lattice(12, m=32, seed=LATTICE_SEED)


def owners_of_roots(info, world):
    return [RR.route_owner(int(k[0]), int(k[1]), int(k[2]), world) for k in info["root_keys"]]
