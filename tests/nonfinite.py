"""Clouds with non-finite points for the extraction's rule "a point with a non-finite x, y or z contributes to nothing" - TEST
INFRASTRUCTURE.

dirty(clean, pattern, seed) INSERTS points with NaN / +inf / -inf coordinates into a clean cloud, so that dirty[finite rows] is the clean
cloud byte for byte and the expected surfels of every case are simply the clean cloud's.  Every inserted point takes the whole record (stamp,
ring, ...) of the clean point it is inserted in front of - points arrive in ascending time - and only the pattern "stamps" departs from that.

Where only one axis is bad, the two other coordinates are those of a clean point whose voxel index on the bad axis is 0, and the point is
inserted right in front of that clean point (the same stamp, so the same temporal cluster): a library that turned the NaN into voxel index 0
would count it into a voxel that is really there.  fault_model() restates that wrong rule as data, for the CPU tests that show every case
to be able to fail (tests/test_nonfinite_ref.py).  Nothing here runs on a GPU."""
import numpy as np

import extract_gates as G
from wildcat_slam_amd import records as R
from wildcat_slam_amd import synth

VS = float(np.float32(0.8))
KTILE = 1024  # kFxTile (csrc/extract_plan.h): the points of one k_fx_acc workgroup, four consecutive ones per lane
VALUES = (np.nan, np.inf, -np.inf)
PATTERNS = ("scatter", "ends-nan", "ends-pinf", "ends-ninf", "runs", "all", "stamps")
CLOUDS = ("lattice0", "room_firing", "shuffled", "wide", "far")
FAR_SHIFT = 450.0


def xyz(pts):
    return np.stack([pts["x"], pts["y"], pts["z"]], 1)


def finite_rows(pts):
    return np.isfinite(xyz(pts)).all(axis=1)


def same_records(a, b):
    """every field bit for bit (the 48-byte record has padding, which a copy need not keep)"""
    return len(a) == len(b) and all(np.ascontiguousarray(a[f]).tobytes() == np.ascontiguousarray(b[f]).tobytes() for f in a.dtype.names)


def voxels(pts):
    """floor(p / vs) in fp64, as the reference forms it (finite points only)"""
    return np.floor(xyz(pts).astype(np.float64) / VS).astype(np.int64)


# ---- clouds ---------------------------------------------------------------------------------------------------------------------------
_CLOUDS = {}


def _lattice0():
    """g2_lattice(60, m=32) translated so that its FIRST root (points 0 .. 255) is voxel (0, 0, 0): that voxel emits surfels, and the
    cloud's first stamps are its"""
    pts, info = synth.g2_lattice(60, m=32)
    off = (-info["root_keys"][0] * np.float64(VS)).astype(np.float32)
    for a, axis in enumerate("xyz"):
        pts[axis] = pts[axis] + off[a]
    return pts


def cloud(name):
    if name not in _CLOUDS:
        if name == "lattice0":
            pts = _lattice0()
        elif name == "room_firing":  # firing order, long record lists, layer 2
            pts = synth.g1_room(60_000)
        elif name == "shuffled":  # no run structure: the unordered / radix point sort
            src = cloud("lattice0")
            pts = src[np.random.default_rng(11).permutation(len(src))]
            pts["time"] = np.sort(src["time"])
        elif name == "wide":  # two groups 2000 m apart: wide keys (test_wide_extent_falls_back_to_wide_keys at a tenth of its points)
            a, _ = synth.g2_lattice(7, m=32, span=8)
            b, _ = synth.g2_lattice(7, m=32, span=8, seed=5, t_start=synth.T0 + 0.6)
            b["x"] += np.float32(2000.0)
            pts = synth.concat_points(a, b)
        elif name == "far":  # 562 root voxels from the frame's origin: the relative keys fit only around one of the cloud's OWN points
            pts = cloud("lattice0").copy()
            pts["x"] = (pts["x"].astype(np.float64) + FAR_SHIFT).astype(np.float32)
        else:
            raise KeyError(name)
        assert finite_rows(pts).all() and np.all(np.diff(pts["time"]) >= 0)
        _CLOUDS[name] = pts
    return _CLOUDS[name]


# ---- insertion ------------------------------------------------------------------------------------------------------------------------
def insert(clean, at, rows):
    """rows[j] (x, y, z) goes in front of clean[at[j]] (at ascending, at[j] == len(clean): behind the last point) with that point's
    record -> (dirty, removed_index: where the inserted points are in dirty)"""
    n, m = len(clean), len(at)
    at = np.asarray(at, np.int64)
    assert m == 0 or (np.all(np.diff(at) >= 0) and at[0] >= 0 and at[-1] <= n)
    out = np.zeros(n + m, R.POINT)
    removed = at + np.arange(m)
    keep = np.ones(n + m, bool)
    keep[removed] = False
    out[keep] = clean
    if m:
        out[removed] = clean[np.minimum(at, n - 1)]
        rows = np.asarray(rows, np.float32)
        out["x"][removed], out["y"][removed], out["z"][removed] = rows[:, 0], rows[:, 1], rows[:, 2]
    assert same_records(out[keep], clean) and not finite_rows(out)[removed].any()
    return out, removed


def _bad_rows(clean, m, rng, near=None):
    """m rows cycling through NaN, +inf, -inf on x, then y, then z, then on all three -> (rows, source): source[j] = the clean point whose
    two other coordinates row j has (its voxel index on the bad axis is 0), or -1.  near: prefer sources next to this clean index"""
    k, p = voxels(clean), xyz(clean)
    rows, src = np.empty((m, 3), np.float32), np.full(m, -1, np.int64)
    # (axis 3: the points of voxel (0, 0, 0), where an all-NaN point would be counted)
    cands = [np.flatnonzero(k[:, a] == 0) for a in range(3)] + [np.flatnonzero((k == 0).all(axis=1))]
    for j in range(m):
        axis, val = (j % 12) // 3, VALUES[j % 3]
        cand = cands[axis]
        if axis == 3:
            rows[j] = val
        if len(cand):
            s = int(cand[rng.integers(len(cand))]) if near is None else int(cand[np.argmin(np.abs(cand - near))])
            src[j] = s
            if axis < 3:
                rows[j] = p[s]
                rows[j, axis] = val
        elif axis < 3:  # no voxel with index 0 on that axis: any clean point's two other coordinates
            rows[j] = p[int(rng.integers(len(clean)))]
            rows[j, axis] = val
    return rows, src


def _scatter(clean, rng):
    n = len(clean)
    m = max(24, n // 100)
    rows, src = _bad_rows(clean, m, rng)
    at = np.where(src >= 0, src, rng.integers(0, n + 1, m))  # in front of its source: the same stamp, the same temporal cluster
    order = np.argsort(at, kind="stable")
    return at[order], rows[order]


def _runs(clean, rng):
    """(dirty start, length): a whole k_fx_acc tile, 2048 + 3 from an odd index, and 1, 2 and 3 inside one lane's four points"""
    n = len(clean)
    assert n >= 3 * KTILE
    spans = [(KTILE, KTILE), (3 * KTILE + 1, 2 * KTILE + 3)]
    base = 6 * KTILE + 4 * ((n - 3 * KTILE) // 8)  # (a multiple of 4, behind both long runs)
    spans += [(base + 1, 1), (base + 4 * 9 + 1, 2), (base + 4 * 20 + 1, 3)]
    at, rows, done = [], [], 0
    for start, length in spans:
        a = start - done
        assert 0 <= a <= n
        r, _ = _bad_rows(clean, length, rng, near=a)
        at += [a] * length
        rows.append(r)
        done += length
    return np.array(at), np.concatenate(rows), spans


def _end_rows(clean, val, seed):
    """the rows in front of the first and behind the last clean point.  seed 0: all three coordinates bad.  seed s > 0: one axis,
    (s - 1) % 3, the other two coordinates those of the ((s - 1) // 3)-th earliest (latest) clean point whose voxel index on that axis
    is 0 - early (late) enough, it shares a temporal cluster with the end point, whose stamp is the first (last) clean point's"""
    rows = np.full((2, 3), val, np.float32)
    if seed > 0:
        axis, rank = (seed - 1) % 3, (seed - 1) // 3
        cand = np.flatnonzero(voxels(clean)[:, axis] == 0)
        p = xyz(clean)
        for r, src in enumerate((cand[rank] if len(cand) > rank else 0, cand[-1 - rank] if len(cand) > rank else len(clean) - 1)):
            rows[r] = p[src]
            rows[r, axis] = val
    return rows


def dirty(clean, pattern, seed=0):
    """-> (dirty cloud, removed_index).  dirty[finite rows] is `clean` byte for byte."""
    rng = np.random.default_rng([seed, len(clean)] + [ord(c) for c in pattern])
    n = len(clean)
    if pattern in ("scatter", "stamps"):
        at, rows = _scatter(clean, rng)
        out, removed = insert(clean, at, rows)
        if pattern == "stamps":  # stamps outside the clean cloud's range, every fourth one NaN: a dropped point's stamp raises nothing
            lo, hi = float(clean["time"][0]), float(clean["time"][-1])
            st = np.where(np.arange(len(removed)) % 2 == 0, lo - 1000.0 - np.arange(len(removed)), hi + 1000.0 + np.arange(len(removed)))
            st[3::4] = np.nan
            out["time"][removed] = st
        return out, removed
    if pattern.startswith("ends-"):  # index 0 and index n - 1 of the cloud
        val = dict(nan=np.nan, pinf=np.inf, ninf=-np.inf)[pattern[5:]]
        return insert(clean, [0, n], _end_rows(clean, val, seed))
    if pattern == "runs":
        at, rows, spans = _runs(clean, rng)
        out, removed = insert(clean, at, rows)
        for start, length in spans:  # the runs are where the pattern says they are
            assert not finite_rows(out)[start:start + length].any() and finite_rows(out)[start - 1] and finite_rows(out)[start + length]
        return out, removed
    if pattern == "all":  # every point non-finite (the stamps stay the clean cloud's)
        out = clean.copy()
        rows, _ = _bad_rows(clean, n, rng)
        out["x"], out["y"], out["z"] = rows[:, 0], rows[:, 1], rows[:, 2]
        return out, np.arange(n)
    raise KeyError(pattern)


_CASES = {}


def case(cloud_name, pattern):
    """(clean: the cloud without the dirty points, dirty, removed_index), built once per process"""
    key = (cloud_name, pattern)
    if key not in _CASES:
        clean = cloud(cloud_name)
        d, removed = dirty(clean, pattern, SEEDS.get(key, 0))
        _CASES[key] = (clean[:0] if pattern == "all" else clean, d, removed)  # (all: what is left is the empty cloud)
    return _CASES[key]


# (cloud, pattern) -> seed, where seed 0 gave a case the fault model passes (tests/test_nonfinite_ref.py holds that it no longer does).
# The ends with all three coordinates bad land in voxel (0, 0, 0), which is empty air in these three clouds: one bad axis instead, next
# to an early (late) point of a voxel whose index on that axis is 0.
SEEDS = {(c, "ends-" + v): sd for c, sd in (("room_firing", 5), ("shuffled", 1), ("wide", 1)) for v in ("nan", "pinf", "ninf")}


def cases():
    """the (cloud, pattern) pairs of the tests: every pattern on every cloud"""
    return [(c, p) for c in CLOUDS for p in PATTERNS]


# ---- the wrong rule, as data ----------------------------------------------------------------------------------------------------------
def fault_model(pts, only_nan=False):
    """what a bare float -> int conversion on the device makes of these points: a NaN coordinate is voxel index 0 (here: the centre of
    voxel 0 on that axis), +-inf saturates (here: +-(2^20 vs), beyond every key range).  only_nan: the points with an infinite coordinate
    are left out - what the NaN points alone do."""
    p = xyz(pts)
    if only_nan:
        pts = pts[~np.isinf(p).any(axis=1)]
        p = xyz(pts)
    out = pts.copy()
    q = np.where(np.isnan(p), np.float32(0.5 * VS), p)
    q = np.where(np.isinf(q), np.sign(q) * np.float32(2.0**20 * VS), q).astype(np.float32)
    out["x"], out["y"], out["z"] = q[:, 0], q[:, 1], q[:, 2]
    return out


def key_extent(pts):
    """the largest |voxel index - point 0's| over the cloud: <= 511 fits the 32-bit keys (and the default path), < 2^20 the wide ones,
    beyond that the library returns WC_ERR_ARG"""
    k = voxels(pts)
    return int(np.abs(k - k[0]).max()) if len(k) else 0


# ---- the count gates ------------------------------------------------------------------------------------------------------------------
GATE_K = (0, 3, 2)  # a root whose x index is 0
GATES = ("root-20", "root-21", "l1-19", "l1-20")


def gate(name):
    """one planar patch of n finite points at a count gate, and five points (NaN, y, z) on its plane with stamps inside it:
      root-20 / root-21   the root is tested when n > min_points (20): 20 points stay untested, and 25 would not
      l1-19 / l1-20       a layer-1 node's temporal cluster is kept when n >= cluster_min_points (20): 19 are dropped, and 24 would not be
                          (the node holds a second cluster of 40 points 0.1 s later, so it is tested; the root is no plane)
    The layer-1 site is the child (-, +, +): a NaN fails the octant test x > centre, as it fails every comparison.
    -> dict(clean, dirty, removed, emits: the site gives a surfel in the clean cloud)"""
    if name in _CASES:
        return _CASES[name]
    site, n = name.split("-")
    n = int(n)
    rng = np.random.default_rng([7] + [ord(c) for c in name])
    k = GATE_K
    flip = np.array([-1.0, 1.0, 1.0]) if site == "l1" else np.ones(3)
    u = G._flat(rng, site, n) * flip
    patch = G.world(k, u)
    t_end = G.T0 + 1e-3 + G.DT * n
    parts = G._fillers(rng, k) + [(patch, G._stamps(n, t_end))]
    if site == "l1":
        parts.append((G.world(k, G._corners(rng, "root") * flip), G._stamps(20, t_end)))
        parts.append((G.world(k, G._flat(rng, "l1", 40) * flip), G._stamps(40, t_end + 0.1 + 40 * G.DT)))
    clean = G._assemble(parts)
    mem = G._members_of(patch)(clean)
    assert len(mem) == n
    extra = G.world(k, G._flat(rng, site, 5) * flip)  # on the patch's plane, inside the site's cell
    extra[:, 0] = np.nan
    d, removed = insert(clean, mem[2:7], extra)
    _CASES[name] = dict(name=name, clean=clean, dirty=d, removed=removed, site=site, n=n, emits=name in ("root-21", "l1-20"))
    return _CASES[name]
