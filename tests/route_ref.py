"""Plain restatement of the routed cloud's index work (csrc/route.hip): the owner hash, the root voxel index, the stable
partition by owner and the k-way surfel merge.  It takes NOTHING from the library under test - the hash is Python integers
masked to 64 bits, the voxel index numpy float64, the orders Python's sorted() - so that a test built on it notices a library
whose hash, voxel rule, partition or merge changed together with its own host helpers (dist.route_partition_host takes the hash
from wc_route_owner).  tests/test_route_ref.py holds it to the library's host side and to the oracle without a GPU."""
import numpy as np

M32, M64 = (1 << 32) - 1, (1 << 64) - 1
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1

# known answers: (kx, ky, kz) -> hash mod 64, and the first three hashes in full (recorded from the C++ function once)
KNOWN_KEYS = [(0, 0, 0), (-1, -1, -1), (INT32_MIN, 0, 5), (INT32_MAX, INT32_MIN, 1), (1, 2, 3), (-7, 12, -300), (INT32_MIN,) * 3]
KNOWN_OWNERS_64 = [0, 39, 55, 46, 41, 56, 63]
KNOWN_HASHES = [0, 2508094951, 1757303095]


def route_hash(kx, ky, kz):
    """the 32-bit hash of a root voxel index: the three int32 as unsigned words, multiplied into 64 bits, one xor-shift-multiply round"""
    h = ((int(kx) & M32) * 0x9E3779B97F4A7C15) & M64
    h ^= ((int(ky) & M32) * 0xC2B2AE3D27D4EB4F) & M64
    h ^= ((int(kz) & M32) * 0x165667B19E3779F9) & M64
    h ^= h >> 29
    h = (h * 0xBF58476D1CE4E5B9) & M64
    h ^= h >> 32
    return h & M32


def route_owner(kx, ky, kz, world):
    return route_hash(kx, ky, kz) % int(world)


def route_voxel(xyz_f32, voxel_f32):
    """(n, 3) float32 coordinates -> (n, 3) int32 root voxel indices: floor(float64(p) / float64(float32(voxel))) per axis, INT32_MIN
    where the quotient is not finite or lies outside [-2^31, 2^31 - 1]"""
    p = np.asarray(xyz_f32, np.float32).reshape(-1, 3).astype(np.float64)
    v = np.float64(np.float32(voxel_f32))
    with np.errstate(all="ignore"):
        f = np.floor(p / v)
        ok = np.isfinite(f) & (f >= -2147483648.0) & (f <= 2147483647.0)
    out = np.full(f.shape, INT32_MIN, np.int64)
    out[ok] = f[ok].astype(np.int64)
    return out.astype(np.int32)


def hashes_of(keys):
    """(n, 3) voxel indices -> list of n Python-integer hashes (each distinct key hashed once)"""
    memo = {}
    out = []
    for k in map(tuple, np.asarray(keys, np.int64).reshape(-1, 3).tolist()):
        h = memo.get(k)
        if h is None:
            h = memo[k] = route_hash(*k)
        out.append(h)
    return out


def owners_of(xyz_f32, voxel_f32, world):
    """owner of every point -> int array of length n"""
    return np.array([h % int(world) for h in hashes_of(route_voxel(xyz_f32, voxel_f32))], np.int64).reshape(-1)


def xyz_of(points):
    """(n, 3) float32 of a POINT (or any x / y / z) record array"""
    return np.stack([points["x"], points["y"], points["z"]], 1).astype(np.float32)


def partition_ref(points, voxel, world, hashes=None):
    """-> per owner the source indices of its points, in source order (hashes: hashes_of() of the cloud's voxels, to share
    between calls that differ in `world` only)"""
    if hashes is None:
        hashes = hashes_of(route_voxel(xyz_of(points), voxel))
    segs = [[] for _ in range(int(world))]
    for i, h in enumerate(hashes):
        segs[h % int(world)].append(i)
    return [np.array(s, np.int64) for s in segs]


def keys_owned_by(world, start=0):
    """one voxel index (kx, 0, 0), kx >= start, per rank of `world`: the first the search meets -> (world, 3) int64"""
    found, kx = {}, int(start)
    while len(found) < world:
        found.setdefault(route_owner(kx, 0, 0, world), (kx, 0, 0))
        kx += 1
    return np.array([found[r] for r in range(world)], np.int64)


def merge_ref(lists, id_lists=None):
    """k time-sorted SURFEL lists (and their SURFEL_ID lists, or None) -> the merged order as (list index, position) pairs, by a plain
    sorted(): with ids the key is (t, kx, ky, kz, node as unsigned, list index, position), without (t, list index, position)"""
    keys = []
    for j, s in enumerate(lists):
        t = [float(x) for x in s["t"]]
        if id_lists is None:
            keys += [(t[p], j, p) for p in range(len(s))]
        else:
            i = id_lists[j]
            assert len(i) == len(s)
            keys += [(t[p], int(i["kx"][p]), int(i["ky"][p]), int(i["kz"][p]), int(i["node"][p]) & M32, j, p) for p in range(len(s))]
    return [(k[-2], k[-1]) for k in sorted(keys)]


def take(lists, order, dtype):
    """the records of `lists` in the order of merge_ref() -> one array"""
    out = np.zeros(len(order), dtype)
    for n, (j, p) in enumerate(order):
        out[n] = lists[j][p]
    return out
