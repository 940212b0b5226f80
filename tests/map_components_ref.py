"""Connected components of the voxel map (include/wildcat_hip.h: wc_map_components, wc_map_remove_small, wc_map_label_keys)
without a GPU and without the library.

1. `components` is the restatement: a plain dict of voxel indices and a breadth-first search in Python integers, then the numbering, label
   and record rules of the header.  `fault` switches ONE deliberate mistake in:
     "wrap"            a neighbour index past the end of the key range wraps to the other end instead of not existing
     "upper_forgotten" the search follows the lexicographically lower neighbours only
     "gate_one_end"    min_points is tested on the voxel an edge starts from and not on the one it reaches
     "first_seen"      components are numbered as a scan in (kz, ky, kx) order first sees them, not by their root
2. `brute` is an independent check of the partition: the all-pairs adjacency matrix and its closure.
3. `remove_small` restates wc_map_remove_small on top of `components`.
4. The planted shapes of the tests.  Every shape is (keys (n, 3) int64 in ascending order, counts (n,) int64)."""
import collections

import numpy as np

KEY_LIM = 1 << 20  # |k| < 2^20
L = KEY_LIM - 1  # the largest voxel index; -L is the smallest
NO_COMPONENT = 0xFFFFFFFF
COMPONENT = np.dtype([("first", "u4"), ("voxels", "u4"), ("points", "u8"), ("kmin", "i4", 3), ("kmax", "i4", 3)])  # wc_map_component
FAULTS = ("wrap", "upper_forgotten", "gate_one_end", "first_seen")
OUT = ("voxels", "nodes", "components", "largest")


def offsets(connectivity):
    """the 6 / 18 / 26 offsets: max |d| == 1 and sum |d| <= 1 / 2 / 3"""
    c = {6: 1, 18: 2, 26: 3}[connectivity]
    r = (-1, 0, 1)
    return [(x, y, z) for x in r for y in r for z in r if (x, y, z) != (0, 0, 0) and abs(x) + abs(y) + abs(z) <= c]


def sort_keys(keys, counts=None):
    """rows in ascending (kx, ky, kz) order -> (keys int64, counts int64; one point each without counts)"""
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    counts = np.ones(len(keys), np.int64) if counts is None else np.asarray(counts, np.int64).reshape(-1)
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    return keys[order], counts[order]


def components(keys, counts, connectivity=26, min_points=1, fault=None):
    """keys (n, 3) strictly ascending, counts (n,) -> (labels (n,) uint32, COMPONENT array, dict(voxels, nodes, components, largest))"""
    assert fault is None or fault in FAULTS
    assert min_points >= 1
    keys = [tuple(int(x) for x in k) for k in np.asarray(keys).reshape(-1, 3)]
    counts = [int(c) for c in np.asarray(counts).reshape(-1)]
    assert all(a < b for a, b in zip(keys, keys[1:])), "keys are strictly ascending"
    assert all(-KEY_LIM < x < KEY_LIM for k in keys for x in k)
    index = {k: i for i, k in enumerate(keys)}
    node = [c >= min_points for c in counts]
    offs = offsets(connectivity)
    if fault == "upper_forgotten":
        offs = [d for d in offs if d < (0, 0, 0)]

    def neighbour(k, d):
        q = [a + b for a, b in zip(k, d)]
        if fault == "wrap":
            q = [(x + L) % (2 * L + 1) - L for x in q]
        return tuple(q) if all(-KEY_LIM < x < KEY_LIM for x in q) else None

    comp_of = [None] * len(keys)  # the index of the voxel the search started from
    seeds = range(len(keys))
    if fault == "first_seen":
        seeds = sorted(seeds, key=lambda i: keys[i][::-1])
    members = collections.OrderedDict()
    for s in seeds:
        if not node[s] or comp_of[s] is not None:
            continue
        comp_of[s] = s
        todo, found = collections.deque([s]), [s]
        while todo:
            i = todo.popleft()
            for d in offs:
                q = neighbour(keys[i], d)
                j = index.get(q) if q is not None else None
                if j is None or comp_of[j] is not None or not (node[j] or fault == "gate_one_end"):
                    continue
                comp_of[j] = s
                todo.append(j)
                found.append(j)
        members[s] = found
    # numbering: by root, the member of smallest key (= smallest index); the fault keeps the order of discovery
    groups = list(members.values())
    if fault != "first_seen":
        groups.sort(key=min)
    labels = np.full(len(keys), NO_COMPONENT, np.uint32)
    comps = np.zeros(len(groups), COMPONENT)
    for c, g in enumerate(groups):
        labels[g] = c
        k = np.array([keys[i] for i in g], np.int64)
        comps[c] = (min(g), len(g), sum(counts[i] for i in g), tuple(k.min(0)), tuple(k.max(0)))
    out = dict(voxels=len(keys), nodes=int(np.sum(labels != NO_COMPONENT)), components=len(groups),
               largest=max((len(g) for g in groups), default=0))
    return labels, comps, out


def brute(keys, counts, connectivity=26, min_points=1):
    """the partition by the all-pairs adjacency matrix and its closure -> labels (n,) uint32 numbered by smallest member"""
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    node = np.asarray(counts).reshape(-1) >= min_points
    d = np.abs(keys[:, None, :] - keys[None, :, :])
    adj = (d.max(-1) == 1) & (d.sum(-1) <= {6: 1, 18: 2, 26: 3}[connectivity]) & node[:, None] & node[None, :]
    reach = adj | np.eye(len(keys), dtype=bool)
    while True:
        nxt = (reach.astype(np.int64) @ reach.astype(np.int64)) > 0
        if np.array_equal(nxt, reach):
            break
        reach = nxt
    root = np.argmax(reach, axis=1)  # (the first reachable index: the smallest member)
    labels = np.full(len(keys), NO_COMPONENT, np.uint32)
    roots = np.unique(root[node])
    labels[node] = np.searchsorted(roots, root[node])
    return labels


def remove_small(keys, counts, min_voxels, min_comp_points=0, connectivity=26, min_points=1, drop_sparse=False):
    """wc_map_remove_small -> (keep (n,) bool, dict(components, components_removed, voxels_removed, points_removed))"""
    counts = np.asarray(counts, np.int64).reshape(-1)
    labels, comps, out = components(keys, counts, connectivity, min_points)
    small = np.array([(min_voxels and int(c["voxels"]) < min_voxels) or (min_comp_points and int(c["points"]) < min_comp_points) for c in comps], bool)
    gone = np.zeros(len(counts), bool)
    is_node = labels != NO_COMPONENT
    gone[is_node] = small[labels[is_node]] if len(small) else False
    if drop_sparse:
        gone |= ~is_node
    return ~gone, dict(components=out["components"], components_removed=int(small.sum()), voxels_removed=int(gone.sum()),
                       points_removed=int(counts[gone].sum()))


# ---- planted shapes -------------------------------------------------------------------------------------------------------------
PAIRS = {"face": (1, 0, 0), "edge": (0, 1, 1), "corner": (1, 1, 1), "apart": (0, 2, 0)}
# connected? per (pair, connectivity): the 12 verdicts
PAIR_VERDICTS = {("face", 6): True, ("face", 18): True, ("face", 26): True, ("edge", 6): False, ("edge", 18): True, ("edge", 26): True,
                 ("corner", 6): False, ("corner", 18): False, ("corner", 26): True, ("apart", 6): False, ("apart", 18): False, ("apart", 26): False}


def pair(kind, at=(3, -2, 7)):
    a = np.array(at, np.int64)
    return sort_keys([a, a + np.array(PAIRS[kind])])


def range_ends():
    """voxels at k = L and k = -L (the ends of the key range) on each axis: alone on one row - nothing joins across the range's ends -,
    with a partner one step inside on another row, the two far corners, and voxels whose z is at one end while y differs by one - nothing
    joins across axes"""
    rows = []
    for a in range(3):
        e, b = np.eye(3, dtype=np.int64)[a], np.eye(3, dtype=np.int64)[(a + 1) % 3]
        rows += [e * L, -e * L]  # alone, at both ends of one row
        rows += [e * L + 10 * b, e * (L - 1) + 10 * b, -e * L + 10 * b, -e * (L - 1) + 10 * b]  # with a partner one step inside
    rows += [np.array([L, L, L]), np.array([L, L, L - 1]), np.array([-L, -L, -L]), np.array([-L + 1, -L + 1, -L + 1])]
    rows += [np.array([0, 5, L]), np.array([0, 6, -L]), np.array([7, L, 0]), np.array([8, -L, 0])]
    return sort_keys(rows)


def snake(width=100, rows=30):
    """a 6-connected chain that folds back and forth in the plane z = 0: rows y = 0, 2, 4, ... of `width` voxels along x, joined at
    alternating ends -> (keys, counts, chain: the indices into keys along the chain)"""
    path = []
    for r in range(rows):
        xs = range(width) if r % 2 == 0 else range(width - 1, -1, -1)
        path += [(x, 2 * r, 0) for x in xs]
        if r + 1 < rows:
            path.append((path[-1][0], 2 * r + 1, 0))
    keys, counts = sort_keys(path)
    index = {tuple(k): i for i, k in enumerate(keys.tolist())}
    return keys, counts, np.array([index[p] for p in path])


def comb(teeth=40, length=60):
    """`teeth` rows along x (y = 0, 2, 4, ...) that start at x = 0 - where the small keys are - and are joined only by a spine at x = length"""
    rows = [(x, 2 * t, 0) for t in range(teeth) for x in range(length)]
    rows += [(length, y, 0) for y in range(2 * teeth - 1)]
    return sort_keys(rows)


def block(side=12):
    r = np.arange(side)
    return sort_keys(np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3) - 5)


def checker(side=16):
    """the voxels of a side^3 cube with even kx + ky + kz: no two share a face; every one shares an edge with others"""
    k = block(side)[0]
    return sort_keys(k[k.sum(1) % 2 == 0])


def bridge():
    """two 3^3 blobs of three-point voxels joined by ONE one-point voxel -> (keys, counts, index of the bridge voxel)"""
    r = np.arange(3)
    blob = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    keys = np.concatenate([blob, [[3, 1, 1]], blob + np.array([4, 0, 0])])
    counts = np.concatenate([np.full(27, 3), [1], np.full(27, 3)])
    keys, counts = sort_keys(keys, counts)
    return keys, counts, int(np.flatnonzero(counts == 1)[0])


def z_major_pair():
    """two single voxels whose order by (kx, ky, kz) is the reverse of their order by (kz, ky, kx)"""
    return sort_keys([(0, 0, 5), (1, 0, 0)])


def random_sparse(seed, n, fill=0.2, max_count=4):
    """n distinct voxels in a cube about 1 / fill times as large, counts 1 .. max_count"""
    rng = np.random.Generator(np.random.PCG64(seed))
    side = max(int(np.ceil((n / fill) ** (1 / 3))), 2)
    cells = rng.permutation(side**3)[:n]
    keys = np.stack([cells // (side * side), (cells // side) % side, cells % side], -1) - side // 2
    return sort_keys(keys, rng.integers(1, max_count + 1, n))


def planted():
    """name -> (keys, counts) of every planted shape"""
    out = {"single": sort_keys([(4, -9, 2)]), "range_ends": range_ends(), "snake": snake()[:2], "comb": comb(), "block": block(),
           "checker": checker(), "bridge": bridge()[:2], "z_major_pair": z_major_pair(), "empty": sort_keys(np.zeros((0, 3)))}
    for kind in PAIRS:
        out["pair_" + kind] = pair(kind)
    return out
