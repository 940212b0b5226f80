"""The voxel map's removal in place (include/wildcat_hip.h: wc_map_carve_remove, wc_map_remove_keys) without a GPU.

1. The reference for a removal is "the map of the surviving points": `Survivors` keeps the points inserted so far and drops those whose
   voxel a call removes - the expected export and state are then map_carve_ref.voxels_of / map_state_ref.state_of of what is left, and on
   the GPU a fresh map of those points.  It sits on top of map_carve_ref and map_state_ref and edits neither.
2. `Table` is a small model of the open-addressing table (csrc/map.hip): map_hash restated (the splitmix64 finaliser on the packed key),
   insert, find, remove-to-tombstone, compact, rehash and the room policy of csrc/map_room.h.  `fault` switches ONE deliberate mistake in:
     "find_stops_at_tomb"   the read-only probe ends at a tombstone as if it were empty
     "compact_emits_tombs"  the compaction takes a tombstone for an occupied slot
     "rehash_carries_tombs" a replacement moves the tombstones into the new table (they are one key: they collapse into one slot, which
                            the model's tombstones() - a count in the table itself - shows; on the device no map output would)
     "counters_stay"        a removal does not take the voxel and its points off the counters
     "bound_ignores_tombs"  the room policy does not count the tombstones
3. `cluster_keys` returns voxel indices that share one home slot under a mask."""
import numpy as np

import map_carve_ref as CR
import map_state_ref as MS
from map_query_ref import KEY_LIM, pack

EMPTY, TOMB = 2**64 - 1, 2**64 - 2
MASK64 = 2**64 - 1
KEEP, GROW, PURGE, FULL = 0, 1, 2, -1
MAX_CAP = 2**32
FAULTS = ("find_stops_at_tomb", "compact_emits_tombs", "rehash_carries_tombs", "counters_stay", "bound_ignores_tombs")


def map_hash(k):
    """splitmix64 finaliser, one Python integer"""
    k = int(k) & MASK64
    k ^= k >> 30
    k = (k * 0xBF58476D1CE4E5B9) & MASK64
    k ^= k >> 27
    k = (k * 0x94D049BB133111EB) & MASK64
    k ^= k >> 31
    return k


def map_hash_np(k):
    """the same on a uint64 array (the products wrap)"""
    k = np.asarray(k).astype(np.uint64)
    k = k ^ (k >> np.uint64(30))
    k = k * np.uint64(0xBF58476D1CE4E5B9)
    k = k ^ (k >> np.uint64(27))
    k = k * np.uint64(0x94D049BB133111EB)
    return k ^ (k >> np.uint64(31))


def cluster_keys(count, mask, span=2**20):
    """`count` voxel indices (kx, 0, 0), 0 <= kx < span, whose packed keys have ONE home slot under `mask` (the fullest one) -> (count, 3) int32"""
    kx = np.arange(span, dtype=np.int64)
    keys = np.stack([kx, np.zeros_like(kx), np.zeros_like(kx)], -1)
    home = (map_hash_np(pack(keys)) & np.uint64(mask)).astype(np.int64)
    slot = int(np.bincount(home, minlength=mask + 1).argmax())
    found = kx[home == slot][:count]
    assert len(found) == count, "the span holds too few keys of one home slot"
    return keys[found].astype(np.int32)


def pow2_at_least(x):
    c = 1
    while c < x:
        c <<= 1
    return c


def room(cap, live_bound, tombs, n):
    """csrc/map_room.h restated -> (decision, slots afterwards)"""
    need = 2 * (live_bound + n)
    if need + 2 * tombs <= cap:
        return KEEP, cap
    if need > MAX_CAP:
        return FULL, cap
    want = pow2_at_least(need)
    return (PURGE, cap) if want <= cap else (GROW, want)


def room_before(cap, bound, n):
    """the growth policy as it stood before voxels could be removed (map_make_room) -> (decision, slots afterwards)"""
    need = 2 * (bound + n)
    if need <= cap:
        return KEEP, cap
    want = pow2_at_least(need)
    return (FULL, cap) if want > MAX_CAP else (GROW, want)


def in_range(keys):
    k = np.asarray(keys, np.int64).reshape(-1, 3)
    return np.all((k > -KEY_LIM) & (k < KEY_LIM), axis=1)


class Survivors:
    """the points a map holds: every insert appends, every removal drops the points of the removed voxels"""

    def __init__(self, v):
        self.v = v
        self.points = np.zeros((0, 3), np.float32)

    def insert(self, xyz):
        self.points = np.concatenate([self.points, np.asarray(xyz, np.float32).reshape(-1, 3)])

    def voxels(self):
        """-> (keys (n, 3) ascending, counts (n,))"""
        if not len(self.points):
            return np.zeros((0, 3), np.int64), np.zeros(0, np.int64)
        return CR.voxels_of(self.points, self.v)

    def state(self, moments=True):
        return MS.state_of(self.points, self.v, moments)

    def remove(self, keys):
        """wc_map_remove_keys -> dict(voxels_removed, points_removed, keys_unused); duplicates, absent and out-of-range keys are unused"""
        keys = np.asarray(keys, np.int64).reshape(-1, 3)
        ok = in_range(keys)
        want = np.unique(pack(keys[ok]))
        pk = pack(CR.point_keys(self.points, self.v)) if len(self.points) else np.zeros(0, np.int64)
        gone = np.isin(pk, want)
        vox = len(np.unique(pk[gone]))
        self.points = self.points[~gone]
        return dict(voxels_removed=vox, points_removed=int(gone.sum()), keys_unused=len(keys) - vox)

    def carve_remove(self, rays, origin, max_range, min_range=0.0, shell=1, min_rays=1, max_steps=4096):
        """wc_map_carve_remove -> (the counting call's dict, the keys (m, 3) it removed)"""
        keys, cnt = self.voxels()
        keep, res = CR.carve(keys, cnt, rays, origin, self.v, max_range, min_range, shell, min_rays, max_steps)
        gone = np.asarray(keys)[~keep]
        if len(gone):
            got = self.remove(gone)
            assert got["voxels_removed"] == res["voxels_removed"] and got["points_removed"] == res["points_removed"]
        return res, gone


class Table:
    """the table of csrc/map.hip, one Python integer per key word and a point count per slot"""

    def __init__(self, cap, fault=None):
        assert fault is None or fault in FAULTS
        self.cap, self.fault = cap, fault
        self.keys, self.cnt = [EMPTY] * cap, [0] * cap
        self.occ = self.pts = 0  # the map's counters (wc_map_size)
        self.host_tombs = 0  # the host's count, the one the room policy sees
        self.growths = self.purges = 0

    def _slot(self, key):
        """map_slot: passes every foreign key, tombstones included, and claims the first empty slot"""
        h = map_hash(key) & (self.cap - 1)
        for _ in range(self.cap):
            if self.keys[h] == EMPTY:
                self.keys[h] = key
                return h, True
            if self.keys[h] == key:
                return h, False
            h = (h + 1) & (self.cap - 1)
        raise AssertionError("no slot: the growth invariant is broken")

    def find(self, key):
        """map_find_from -> slot or -1"""
        h = map_hash(key) & (self.cap - 1)
        for _ in range(self.cap):
            c = self.keys[h]
            if c == key:
                return h
            if c == EMPTY or (c == TOMB and self.fault == "find_stops_at_tomb"):
                return -1
            h = (h + 1) & (self.cap - 1)
        return -1

    def _replace(self, cap):
        old_keys, old_cnt = self.keys, self.cnt
        self.cap, self.keys, self.cnt = cap, [EMPTY] * cap, [0] * cap
        for key, c in zip(old_keys, old_cnt):
            if key == EMPTY or (key == TOMB and self.fault != "rehash_carries_tombs"):
                continue
            h, _ = self._slot(key)  # (a carried tombstone is a key like any other here: they all land in one slot)
            self.cnt[h] = c
        self.host_tombs = 0

    def make_room(self, n):
        tombs = 0 if self.fault == "bound_ignores_tombs" else self.host_tombs
        what, cap = room(self.cap, self.occ, tombs, n)
        assert what != FULL
        if what != KEEP:
            self._replace(cap)
            if what == GROW:
                self.growths += 1
            else:
                self.purges += 1

    def insert(self, keys, counts=None):
        """packed keys, one point each unless counts says otherwise (an insert of sum(counts) points)"""
        keys = [int(k) for k in keys]
        counts = [1] * len(keys) if counts is None else [int(c) for c in counts]
        self.make_room(sum(counts))
        for key, c in zip(keys, counts):
            h, fresh = self._slot(key)
            self.cnt[h] = c if fresh else self.cnt[h] + c  # (a claimed slot starts from zero: its old payload is not reachable)
            self.occ += 1 if fresh else 0
            self.pts += c

    def remove(self, voxel_keys):
        """k_map_remove_keys on (n, 3) voxel indices -> dict of the three counts"""
        voxel_keys = np.asarray(voxel_keys, np.int64).reshape(-1, 3)
        ok = in_range(voxel_keys)
        nv = npts = nn = 0
        for key3, good in zip(voxel_keys, ok):
            h = self.find(int(pack(key3[None])[0])) if good else -1
            if h < 0:
                nn += 1
                continue
            self.keys[h] = TOMB
            nv += 1
            npts += self.cnt[h]
        if self.fault != "counters_stay":
            self.occ -= nv
            self.pts -= npts
        self.host_tombs += nv
        return dict(voxels_removed=nv, points_removed=npts, keys_unused=nn)

    def export(self):
        """k_map_compact and the sort -> (packed keys ascending, counts)"""
        rows = sorted((k, c) for k, c in zip(self.keys, self.cnt) if k != EMPTY and (k != TOMB or self.fault == "compact_emits_tombs"))
        return [k for k, _ in rows], [c for _, c in rows]

    def size(self):
        return self.occ, self.pts

    def tombstones(self):
        """(tombstones in the table now - counted in the table itself -, purges so far)"""
        return sum(1 for k in self.keys if k == TOMB), self.purges


# ---- the cluster scenario of the tests (v = 0.5: every point below is a dyadic number that float32 holds exactly) ---------------------
CLUSTER_V = 0.5
CLUSTER_SLOTS = 8192


def centre_points(keys, off=0.25):
    """one point per voxel index at (k * v + off) on every axis, v = 0.5 -> (n, 3) float32, exact"""
    p = (np.asarray(keys, np.float64).reshape(-1, 3) * CLUSTER_V + off).astype(np.float32)
    assert np.array_equal(CR.point_keys(p, CLUSTER_V), np.asarray(keys, np.int64).reshape(-1, 3))
    return p


def distinct_keys(rng, n, lo, hi, avoid=()):
    """n distinct voxel indices in [lo, hi)^3 that are none of `avoid`"""
    k = rng.integers(lo, hi, (4 * n, 3))
    _, first = np.unique(pack(k), return_index=True)
    k = k[np.sort(first)]
    if len(avoid):
        k = k[~np.isin(pack(k), pack(np.asarray(avoid)))]
    assert len(k) >= n
    return k[:n].astype(np.int32)


def cluster_scenario(seed=11, total=4096):
    """-> dict: cluster (64, 3): one home slot of an 8192-slot table; rest: random voxels, `total` in all; remove_list: every second
    cluster key and a random half of the rest, with duplicates, absent keys and out-of-range keys mixed in, shuffled; removed: its distinct
    present keys; again: a third of `removed`; fresh: voxels the map never held"""
    rng = np.random.Generator(np.random.PCG64(seed))
    cluster = cluster_keys(64, CLUSTER_SLOTS - 1)
    rest = distinct_keys(rng, total - len(cluster), -40, 40, avoid=cluster)
    removed = np.concatenate([cluster[::2], rest[rng.permutation(len(rest))[: len(rest) // 2]]])
    absent = distinct_keys(rng, 50, 100, 140)
    outside = np.array([[KEY_LIM, 0, 0], [0, -KEY_LIM, 0], [0, 0, 2**31 - 1], [-(2**31), 5, 5], [KEY_LIM + 7, -KEY_LIM - 7, 3]], np.int64)
    dup = removed[rng.permutation(len(removed))[:100]]
    remove_list = np.concatenate([removed, absent, outside, dup, dup[:10]]).astype(np.int32)
    remove_list = remove_list[rng.permutation(len(remove_list))]
    again = removed[rng.permutation(len(removed))[: len(removed) // 3]]
    fresh = distinct_keys(rng, 300, 200, 240)
    return dict(cluster=cluster, rest=rest, remove_list=remove_list, removed=removed.astype(np.int32), again=again.astype(np.int32), fresh=fresh)
