"""numpy restatement of the voxel map's ray cast (include/wildcat_hip.h: wc_map_raycast) on an exported map: keys (n, 3) in ascending
(kx, ky, kz) order, counts (n,), centroids (n, 3) float32 - what PointMap.export() returns.  The ray records (cast or not, k0, ke, M) are
map_carve_ref.rays(); the walk is this file's own: the same expressions, and with every position the parameter at which the ray
entered it - the winning t_a of the step that led there, 0.0 for k^(0).

`fault` switches ONE deliberate mistake in, so that the tests can show they would catch it:
  "second_hit"     the second occupied voxel is reported       "shell_off"  end_shell is one too small
  "count_ignored"  min_points is treated as 1                  "t_prev"     t is the parameter of the step before
  "first_off"      first_step is one too large"""
from fractions import Fraction

import numpy as np

import map_carve_ref as CR
from map_query_ref import pack
from wildcat_slam_amd import records as R

RESULT_FIELDS = ("rays_cast", "rays_skipped", "hits", "tested")


def walk_steps_t(P, o, v, k0, ke):
    """the float walk of the rays P (m, 3) from o (one origin, or one per ray), all of them cast: yields (i, active (m,), k (m, 3),
    t (m,)) for i = 0 .. max M: k^(i) of every ray with M >= i and the parameter at which the ray entered it (0.0 for i = 0)"""
    v = np.float64(v)
    k = np.broadcast_to(k0, ke.shape).astype(np.int64).copy()
    M = np.abs(ke - k).sum(1)
    with np.errstate(divide="ignore"):
        inv = 1.0 / (P - o)
    up = (ke > k).astype(np.int64)
    sg = np.sign(ke - k)
    t_in = np.zeros(len(k))
    top = int(M.max()) if len(M) else 0
    for i in range(top + 1):
        yield i, M >= i, k.copy(), t_in.copy()
        cand = (k != ke) & (M > i)[:, None]
        with np.errstate(invalid="ignore", over="ignore"):
            t = ((k + up).astype(np.float64) * v - o) * inv
        ax = np.full(len(k), -1)
        bt = np.zeros(len(k))
        for a in range(3):  # the lowest candidate axis, unless a later one's parameter is strictly smaller
            with np.errstate(invalid="ignore"):
                take = cand[:, a] & ((ax < 0) | (t[:, a] < bt))
            ax = np.where(take, a, ax)
            bt = np.where(take, t[:, a], bt)
        rows = np.nonzero(ax >= 0)[0]
        k[rows, ax[rows]] += sg[rows, ax[rows]]
        t_in = np.where(ax >= 0, bt, t_in)


def walks_t(points, origins, v):
    """the walks of many rays at once, one origin per ray -> (chain (T, m, 3) int64, t (T, m), M (m,)): ray r visits chain[: M[r] + 1, r]
    and enters chain[i, r] at t[i, r]"""
    P = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    o = np.asarray(origins, np.float64).reshape(-1, 3)
    ok_e, ke = CR._keys_of(P, v)
    ok_0, k0 = CR._keys_of(o, v)
    assert ok_e.all() and ok_0.all()
    steps = list(walk_steps_t(P, o, v, k0, ke))
    return np.stack([s[2] for s in steps]), np.stack([s[3] for s in steps]), np.abs(ke - k0).sum(1)


def enter_exact(point, origin, v, chain):
    """the exact rational parameters at which the ray origin -> point enters chain[1], chain[2], ... (chain: its voxels, k^(0) first):
    (b - o_a) / d_a with b = the face between chain[i - 1] and chain[i], v, o and the point taken as the doubles they are"""
    p = [Fraction(float(x)) for x in np.asarray(point, np.float32).reshape(3)]
    o = [Fraction(float(x)) for x in np.asarray(origin, np.float64).reshape(3)]
    vv = Fraction(float(v))
    out = []
    for a_, b_ in zip(chain[:-1], chain[1:]):
        (a,) = [j for j in range(3) if a_[j] != b_[j]]
        out.append((max(int(a_[a]), int(b_[a])) * vv - o[a]) / (p[a] - o[a]))
    return out


def raycast(map_keys, map_counts, map_xyz, points, origin, v, max_range, min_range=0.0, first_step=0, end_shell=0, min_points=1, max_steps=4096,
            fault=None):
    """the call on an exported map -> (hits: R.MAP_RAY_HIT array, one record per point; result: dict of the four counters)"""
    mk = pack(np.asarray(map_keys).reshape(-1, 3))
    assert np.all(mk[1:] > mk[:-1]), "the export is in ascending key order"
    cnt = np.asarray(map_counts, np.int64).reshape(-1)
    cen = np.asarray(map_xyz, np.float32).reshape(-1, 3)
    r = CR.rays(points, origin, v, min_range, max_range, max_steps)
    u = r["used"]
    n, m = len(u), int(u.sum())
    first = int(first_step) + (1 if fault == "first_off" else 0)
    shell = int(end_shell) - (1 if fault == "shell_off" else 0)
    need = 1 if fault == "count_ignored" else int(min_points)
    ke = r["ke"][u]
    row = np.full(m, -1, np.int64)  # the export's row of the hit voxel
    step, tested, t_hit = np.zeros(m, np.int64), np.zeros(m, np.int64), np.full(m, np.inf)
    seen = np.zeros(m, np.int64)  # ("second_hit": occupied tested voxels so far)
    t_before = np.zeros(m)
    for i, active, k, t_in in walk_steps_t(r["P"][u], r["o"], v, r["k0"], ke):
        test = active & (row < 0) & (i >= first) & (np.abs(k - ke).max(1) >= shell)
        tested += test
        occ = np.zeros(m, bool)
        if len(mk):
            pk = pack(k)
            pos = np.minimum(np.searchsorted(mk, pk), len(mk) - 1)
            occ = test & (mk[pos] == pk) & (cnt[pos] >= need)
        if fault == "second_hit":
            seen += occ
            occ = occ & (seen >= 2)
        row = np.where(occ, pos, row) if len(mk) else row
        step = np.where(occ, i, step)
        t_hit = np.where(occ, t_before if fault == "t_prev" else t_in, t_hit)
        t_before = t_in
    hit = row >= 0
    at = np.maximum(row, 0)
    rec = np.zeros(m, R.MAP_RAY_HIT)
    if len(mk):
        rec["xyz"] = np.where(hit[:, None], cen[at], np.float32(0))
        rec["count"] = np.where(hit, cnt[at], 0)
        rec["key"] = np.where(hit[:, None], np.asarray(map_keys, np.int64).reshape(-1, 3)[at], 0)
    rec["t"], rec["step"], rec["tested"] = t_hit, step, tested
    hits = np.zeros(n, R.MAP_RAY_HIT)
    hits["flags"], hits["t"] = 1, np.inf
    hits[u] = rec
    res = dict(rays_cast=m, rays_skipped=n - m, hits=int(hit.sum()), tested=int(tested.sum()))
    return hits, res


def raycast_points(map_points, points, origin, v, max_range=np.inf, **kw):
    """raycast() on the map of map_points, with every voxel's centroid left zero (tests of keys, steps and counts without a device)"""
    keys, cnt = CR.voxels_of(map_points, v) if len(map_points) else (np.zeros((0, 3), np.int64), np.zeros(0, np.int64))
    return raycast(keys, cnt, np.zeros((len(keys), 3), np.float32), points, origin, v, max_range, **kw)
