"""numpy restatement of the voxel map's carving (include/wildcat_hip.h: wc_map_carve): the expressions of the interface, vectorised over
rays in float64, on an exported map's keys.  A second walk in fractions.Fraction - the same voxel keys, exact crossing parameters, ties
to the lowest axis - is what the float walk is held against (test_map_carve_ref.py).

`fault` switches ONE deliberate mistake into the float walk, so that the tests can show they would catch it:
  "stop_early"  the walk's last step is left out        "tie_high"  a tie goes to the highest axis
  "shell_off"   the shell is one voxel too small        "twice"     every voxel seen through is counted twice"""
from fractions import Fraction

import numpy as np

from map_query_ref import KEY_LIM, pack

RESULT_FIELDS = ("rays_used", "rays_skipped", "steps", "voxels_removed", "points_removed")


def _keys_of(x64, v):
    """VoxelLoc per axis -> (in range and finite, floor(x / v) as int64 - 0 where not in range)"""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        kf = np.floor(x64 / np.float64(v))
        ok = np.all((kf > -float(KEY_LIM)) & (kf < float(KEY_LIM)), axis=-1)  # (NaN and inf fail the compares)
    return ok, np.where(ok[..., None], kf, 0.0).astype(np.int64)


def rays(points, origin, v, min_range, max_range, max_steps):
    """what the call says about every point -> dict(P, o, k0, ke, end_ok, used, M)"""
    P = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    o = np.asarray(origin, np.float64).reshape(3)
    end_ok, ke = _keys_of(P, v)
    k0_ok, k0 = _keys_of(o, v)
    with np.errstate(invalid="ignore", over="ignore"):
        d = P - o
        len2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        min2, max2 = np.float64(min_range) * np.float64(min_range), np.float64(max_range) * np.float64(max_range)
        in_range = (len2 >= min2) & (len2 <= max2)
    M = np.abs(ke - k0).sum(1)
    used = end_ok & bool(k0_ok) & in_range & (M <= int(max_steps))
    return dict(P=P, o=o, k0=k0, ke=ke, end_ok=end_ok, used=used, M=np.where(used, M, 0))


def walk_steps(P, o, v, k0, ke, fault=None):
    """the float walk of the rays P (m, 3) from o, all of them used: yields (i, active (m,), k (m, 3)) for i = 0 .. max M: k^(i) of every
    ray with M >= i"""
    v = np.float64(v)
    k = np.broadcast_to(k0, ke.shape).astype(np.int64).copy()
    M = np.abs(ke - k).sum(1)
    if fault == "stop_early":  # (k^(M) is never seen through: the mistake shows in k^(M-1))
        M = M - 2
    with np.errstate(divide="ignore"):
        inv = 1.0 / (P - o)
    up = (ke > k).astype(np.int64)
    sg = np.sign(ke - k)
    top = int(M.max()) if len(M) else 0
    for i in range(top + 1):
        active = M >= i
        yield i, active, k.copy()
        step = M > i
        cand = (k != ke) & step[:, None]
        with np.errstate(invalid="ignore", over="ignore"):
            t = ((k + up).astype(np.float64) * v - o) * inv
        ax = np.full(len(k), -1)
        bt = np.zeros(len(k))
        for a in range(3):  # the lowest candidate axis, unless a later one's parameter is strictly smaller
            with np.errstate(invalid="ignore"):
                wins = (t[:, a] <= bt) if fault == "tie_high" else (t[:, a] < bt)
            take = cand[:, a] & ((ax < 0) | wins)
            ax = np.where(take, a, ax)
            bt = np.where(take, t[:, a], bt)
        rows = np.nonzero(ax >= 0)[0]
        k[rows, ax[rows]] += sg[rows, ax[rows]]


def walk(point, origin, v, fault=None):
    """one ray's voxels k^(0) .. k^(M) as a list of tuples (the float walk)"""
    r = rays(np.asarray(point, np.float32).reshape(1, 3), origin, v, 0.0, np.inf, 1 << 30)
    assert r["used"][0]
    return [tuple(int(x) for x in k[0]) for _, _, k in walk_steps(r["P"], r["o"], v, r["k0"], r["ke"], fault)]


def walks(points, origins, v, fault=None):
    """the float walks of many rays at once, one origin per ray -> (chain (T, m, 3) int64, M (m,)): ray r visits chain[: M[r] + 1, r]"""
    P = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    o = np.asarray(origins, np.float64).reshape(-1, 3)
    ok_e, ke = _keys_of(P, v)
    ok_0, k0 = _keys_of(o, v)
    assert ok_e.all() and ok_0.all()
    return np.stack([k for _, _, k in walk_steps(P, o, v, k0, ke, fault)]), np.abs(ke - k0).sum(1)


def walk_exact(point, origin, v):
    """the same keys, the crossing parameters as exact rationals, ties to the lowest axis -> (voxels, near_tie: at some step two
    candidate parameters differed by at most 2^-48 relative, equal included)"""
    p64 = [float(x) for x in np.asarray(point, np.float32).reshape(3)]
    o64 = [float(x) for x in np.asarray(origin, np.float64).reshape(3)]
    v64 = np.float64(v)
    k0, ke = [int(np.floor(np.float64(x) / v64)) for x in o64], [int(np.floor(np.float64(x) / v64)) for x in p64]  # (the map's keys)
    o, vv = [Fraction(x) for x in o64], Fraction(float(v))
    d = [Fraction(p64[a]) - o[a] for a in range(3)]
    up, sg = [1 if ke[a] > k0[a] else 0 for a in range(3)], [1 if ke[a] > k0[a] else -1 for a in range(3)]
    eps = Fraction(1, 2**48)
    k = list(k0)
    # t_a = ((k_a + up_a) v - o_a) / d_a, exact; only the axis that stepped has a new one
    t = [((k[a] + up[a]) * vv - o[a]) / d[a] if k[a] != ke[a] else None for a in range(3)]
    out, near = [tuple(k)], False
    while k != ke:
        ts = sorted((t[a], a) for a in range(3) if k[a] != ke[a])
        if len(ts) > 1 and abs(ts[1][0] - ts[0][0]) <= abs(ts[0][0]) * eps:
            near = True
        a = ts[0][1]
        k[a] += sg[a]
        if k[a] != ke[a]:
            t[a] = ((k[a] + up[a]) * vv - o[a]) / d[a]
        out.append(tuple(k))
    return out, near


def through_counts(points, origin, v, max_range, min_range=0.0, shell=1, max_steps=4096, fault=None):
    """-> (packed keys seen through, ascending; through(k) of each; packed end-marked keys, ascending; the ray record of rays())"""
    r = rays(points, origin, v, min_range, max_range, max_steps)
    u = r["used"]
    ke = r["ke"][u]
    sh = int(shell) - 1 if fault == "shell_off" else int(shell)
    seen = []
    for _, active, k in walk_steps(r["P"][u], r["o"], v, r["k0"], ke, fault):
        thru = active & (np.abs(k - ke).max(1) > sh)
        seen.append(pack(k[thru]))
    seen = np.concatenate(seen) if seen else np.zeros(0, np.int64)
    keys, cnt = np.unique(seen, return_counts=True)
    if fault == "twice":
        cnt = 2 * cnt
    return keys, cnt, np.unique(pack(r["ke"][r["end_ok"]])), r


def carve(map_keys, map_counts, points, origin, v, max_range, min_range=0.0, shell=1, min_rays=1, max_steps=4096, fault=None, pre=None):
    """the call on an exported map (keys (n, 3), counts (n,)) -> (keep: bool per row, result: dict of the five counters);
    pre: what through_counts() returned for the same points, origin, v, ranges, shell and max_steps (min_rays and the map do not enter it)"""
    mk = pack(np.asarray(map_keys).reshape(-1, 3))
    tk, tc, ek, r = pre if pre is not None else through_counts(points, origin, v, max_range, min_range, shell, max_steps, fault)
    through = np.zeros(len(mk), np.int64)
    if len(tk) and len(mk):
        pos = np.minimum(np.searchsorted(tk, mk), len(tk) - 1)
        through = np.where(tk[pos] == mk, tc[pos], 0)
    marked = np.isin(mk, ek)
    keep = ~((through >= int(min_rays)) & ~marked)
    cnt = np.asarray(map_counts, np.int64).reshape(-1)
    n = len(r["used"])
    res = dict(rays_used=int(r["used"].sum()), rays_skipped=int(n - r["used"].sum()), steps=int(r["M"].sum()),
               voxels_removed=int((~keep).sum()), points_removed=int(cnt[~keep].sum()))
    return keep, res


# ---- the scene of the tests: a box room seen from inside, and phantom points in its free space ----------------------------------------
ROOM_LO, ROOM_HI = np.array([-4.1, -3.1, -0.05]), np.array([4.1, 3.1, 3.05])  # (no wall on a voxel face of the tests' sizes)
ROOM_ORIGIN = np.array([0.25, -0.25, 1.25])  # (a voxel centre at v = 0.5: rays along a diagonal cross two faces at once)


def room_scene(n_az=160, n_el=40, seed=3):
    """-> (sweep (n, 3) float32: one return per direction of a grid on the room's walls, floor and ceiling;
    phantom (m, 3) float32: a blob in free space, a sheet a few centimetres in front of the wall x = 4 and a sheet next to the wall y = 3)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    az = np.linspace(-np.pi, np.pi, n_az, endpoint=False) + 0.01
    el = np.linspace(-1.2, 1.2, n_el)
    A, E = np.meshgrid(az, el)
    d = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], -1).reshape(-1, 3)
    with np.errstate(divide="ignore"):
        s = np.where(d > 0, (ROOM_HI - ROOM_ORIGIN) / d, (ROOM_LO - ROOM_ORIGIN) / d)
    sweep = (ROOM_ORIGIN + s.min(1)[:, None] * d).astype(np.float32)
    blob = np.array([2.0, 1.0, 1.5]) + 0.35 * rng.uniform(-1, 1, (300, 3))
    sheet_x = np.stack([np.full(200, 3.7), rng.uniform(-1.5, 1.5, 200), rng.uniform(0.5, 2.0, 200)], -1)
    sheet_y = np.stack([rng.uniform(-3.0, 0.0, 150), np.full(150, 2.4), rng.uniform(0.5, 2.0, 150)], -1)
    # one return through a window, on the exact diagonal (1, 1, 0): at v = 0.5 every step of its walk is a tie.  Beyond the wall no other
    # ray passes, so the phantom points beside the diagonal - in the voxels an x-first and a y-first walk visit - go or stay by this ray
    sweep = np.concatenate([sweep, (ROOM_ORIGIN + np.array([[6.0, 6.0, 0.0]])).astype(np.float32)])
    beside = np.array([[(0.5 * (j + 1) + 0.25, 0.5 * (j - 1) + 0.25, 1.25), (0.5 * j + 0.25, 0.5 * j + 0.25, 1.25)] for j in (9, 10)]).reshape(-1, 3)
    phantom = np.concatenate([blob, sheet_x, sheet_y, beside]).astype(np.float32)
    return sweep, phantom


def point_keys(points, v):
    """(n, 3) float32 -> voxel indices (n, 3) int64 of finite, in-range points"""
    ok, k = _keys_of(np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64), v)
    assert ok.all()
    return k


def voxels_of(points, v):
    """-> (keys (n, 3) ascending, counts (n,)) of the map of these points"""
    k = point_keys(points, v)
    pk, first, cnt = np.unique(pack(k), return_index=True, return_counts=True)
    return k[first], cnt
