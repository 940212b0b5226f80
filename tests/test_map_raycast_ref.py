"""The restatement of wc_map_raycast (map_raycast_ref.py) on its own, without a GPU: its walk against map_carve_ref's, hand-worked rays,
the hit counts of the room scene, the entering parameter against the exact rational one, the counters, the link to the carve's
"seen through", and a demonstration that the byte comparison the GPU test makes tells each of five mistakes from the right answer."""
import itertools
from fractions import Fraction

import numpy as np
import pytest

import map_carve_ref as CR
import map_raycast_ref as RR

V = 0.5
O = (0.25, 0.25, 0.25)
END_SHELLS, MIN_POINTS, FIRST_STEPS = (0, 1, 2), (1, 3), (0, 1)  # the grid of test_map_raycast_gpu.py's room scene


def _random_rays(n, seed, shift=0.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.uniform(-1, 1, (n, 3)) + shift, (rng.uniform(-8, 8, (n, 3)) + shift).astype(np.float32)


@pytest.fixture(scope="module")
def scene():
    """the room scene once: sweep, phantom, and per v the maps (keys, counts) of sweep + phantom and of the sweep alone"""
    sweep, phantom = CR.room_scene()
    maps = {v: (CR.voxels_of(np.concatenate([sweep, phantom]), v), CR.voxels_of(sweep, v)) for v in (0.5, 0.3)}
    return sweep, phantom, maps


def _cast(m, sweep, v, **kw):
    keys, cnt = m
    return RR.raycast(keys, cnt, np.zeros((len(keys), 3), np.float32), sweep, CR.ROOM_ORIGIN, v, np.inf, **kw)


@pytest.mark.parametrize("v", [0.5, 0.25, 0.3])
def test_walk_is_the_carves_walk(v):
    os_, ps = _random_rays(1000, 5)
    chain, t, M = RR.walks_t(ps, os_, v)
    want, M2 = CR.walks(ps, os_, v)
    assert np.array_equal(chain, want) and np.array_equal(M, M2)
    # the parameters: 0 at k^(0), then non-decreasing along a walk, and the last one at most 1 (the end point lies in ke)
    assert np.all(t[0] == 0.0)
    for r in range(len(M)):
        tr = t[: M[r] + 1, r]
        assert np.all(np.diff(tr) >= -1e-12) and tr[-1] <= 1.0 + 1e-12, (os_[r], ps[r])


@pytest.mark.parametrize("v", [0.5, 0.3])
def test_walk_on_the_room_scene(scene, v):
    sweep, _, _ = scene
    o = np.broadcast_to(CR.ROOM_ORIGIN, sweep.shape)
    chain, t, M = RR.walks_t(sweep, o, v)
    want, M2 = CR.walks(sweep, o, v)
    assert np.array_equal(chain, want) and np.array_equal(M, M2) and M.max() == (24 if v == 0.5 else 40)


def _row(voxels, end=(3.25, 0.25, 0.25), **kw):
    """one ray from O through the voxels {index: count} -> its record"""
    keys = np.array(sorted(voxels), np.int64).reshape(-1, 3)
    cnt = np.array([voxels[k] for k in sorted(voxels)], np.int64)
    hits, res = RR.raycast(keys, cnt, np.zeros((len(keys), 3), np.float32), np.array([end], np.float32), O, V, np.inf, **kw)
    h = hits[0]
    assert res == dict(rays_cast=1, rays_skipped=0, hits=int(h["count"] > 0), tested=int(h["tested"])) and h["flags"] == 0
    return tuple(int(x) for x in h["key"]), int(h["count"]), int(h["step"]), int(h["tested"]), float(h["t"])


def test_hand_cases():
    """a ray along +x from (0.25, 0.25, 0.25) to (3.25, 0.25, 0.25) at v = 0.5: voxels (0..6, 0, 0), the face x = 0.5 i at
    t = (0.5 i - 0.25) * (1 / 3)"""
    third = 1.0 / 3.0
    miss = ((0, 0, 0), 0, 0)
    assert _row({(0, 0, 0): 1}) == ((0, 0, 0), 1, 0, 1, 0.0)  # the origin's own voxel
    assert _row({(1, 0, 0): 2}) == ((1, 0, 0), 2, 1, 2, 0.25 * third)
    assert _row({(6, 0, 0): 1}) == ((6, 0, 0), 1, 6, 7, 2.75 * third)  # ke itself
    assert _row({(6, 0, 0): 1}, end_shell=1) == miss + (6, np.inf) and _row({(5, 0, 0): 1}, end_shell=2) == miss + (5, np.inf)
    assert _row({(5, 0, 0): 1}, end_shell=1) == ((5, 0, 0), 1, 5, 6, 2.25 * third)
    assert _row({(0, 1, 0): 4, (7, 0, 0): 1}) == miss + (7, np.inf) and _row({}) == miss + (7, np.inf)
    # first_step beyond the first occupied voxel: positions 2, 3, 4 are tested
    assert _row({(1, 0, 0): 1, (4, 0, 0): 1}, first_step=2) == ((4, 0, 0), 1, 4, 3, 1.75 * third)
    assert _row({(1, 0, 0): 1}, first_step=2) == miss + (5, np.inf) and _row({(1, 0, 0): 1}, first_step=7) == miss + (0, np.inf)
    # min_points: voxels with fewer points do not stop the ray
    row = {(1, 0, 0): 1, (3, 0, 0): 2, (5, 0, 0): 3}
    assert _row(row, min_points=2) == ((3, 0, 0), 2, 3, 4, 1.25 * third) and _row(row, min_points=3) == ((5, 0, 0), 3, 5, 6, 2.25 * third)
    assert _row(row, min_points=4) == miss + (7, np.inf)
    # the exact diagonal: every step is a tie and goes to x first - (0,0,0) (1,0,0) (1,1,0) (2,1,0) (2,2,0); d = (1, 1, 0), inv = 1
    diag = (1.25, 1.25, 0.25)
    assert _row({(1, 1, 0): 1}, end=diag) == ((1, 1, 0), 1, 2, 3, 0.25) and _row({(2, 1, 0): 1}, end=diag) == ((2, 1, 0), 1, 3, 4, 0.75)
    assert _row({(1, 0, 0): 1, (1, 1, 0): 1}, end=diag) == ((1, 0, 0), 1, 1, 2, 0.25)
    assert _row({(0, 1, 0): 1, (1, 2, 0): 1}, end=diag) == miss + (5, np.inf)  # the voxels a y-first walk would visit


def test_rays_not_cast_by_hand():
    pts = np.array([(3.25, 0.25, 0.25), (np.nan, 0, 0), (0, np.inf, 0), (3e6, 0, 0), (0.25, 0.25, 0.25), (0.25, 2.25, 0.25), (0.25, 9.25, 0.25)],
                   np.float32)
    hits, res = RR.raycast_points(pts[[0, 4, 5, 6]], pts, O, V, max_range=5.0, min_range=1.0, max_steps=5)
    # as map_carve_ref's hand case: only ray 5 is cast (M = 4): NaN, inf, out of range, p = o nearer than min_range, beyond max_range, M = 6 > 5
    assert hits["flags"].tolist() == [1, 1, 1, 1, 1, 0, 1] and res == dict(rays_cast=1, rays_skipped=6, hits=1, tested=1)
    blank = np.zeros(1, RR.R.MAP_RAY_HIT)
    blank["flags"], blank["t"] = 1, np.inf
    assert all(hits[i : i + 1].tobytes() == blank.tobytes() for i in (0, 1, 2, 3, 4, 6))
    assert hits[5]["step"] == 0 and hits[5]["count"] == 1 and hits[5]["t"] == 0.0  # the origin's voxel holds point 4
    far, res = RR.raycast_points(pts[[0]], pts, (3e6, 0, 0), V)
    assert np.all(far["flags"] == 1) and res == dict(rays_cast=0, rays_skipped=7, hits=0, tested=0)


HITS = {  # the room scene: (v, end_shell) -> (hits on the map of sweep + phantom, hits on the map of the sweep alone)
    (0.5, 0): (6401, 6401), (0.5, 1): (1284, 873), (0.5, 2): (335, 1),
    (0.3, 0): (6401, 6401), (0.3, 1): (1662, 1319), (0.3, 2): (320, 1),
}  # fmt: skip


@pytest.mark.parametrize("v", [0.5, 0.3])
def test_room_scene_figures(scene, v):
    sweep, phantom, maps = scene
    assert len(sweep) == 6401 and len(phantom) == 654
    for es in END_SHELLS:
        both, res_b = _cast(maps[v][0], sweep, v, end_shell=es)
        alone, res_a = _cast(maps[v][1], sweep, v, end_shell=es)
        assert (res_b["rays_cast"], res_a["rays_cast"]) == (6401, 6401) and (res_b["hits"], res_a["hits"]) == HITS[v, es]
        for hits, res in ((both, res_b), (alone, res_a)):  # the counters are the records' sums
            assert res["tested"] == int(hits["tested"].sum()) and res["hits"] == int((hits["count"] > 0).sum()) and res["rays_skipped"] == 0
        if es == 0:  # hit steps: every residue mod 8 several hundred times.  The longest walk, the window ray's (M = 24 and 40), is stopped
            # by the wall at step 14 and 22 (at 5 and 9 by the phantom blob); the farthest hits, 18 and 30, are returns in the corners
            for hits in (both, alone):
                st = hits["step"]
                assert (st.min(), st.max()) == ((4, 18) if v == 0.5 else (6, 30)) and np.bincount(st % 8, minlength=8).min() >= 300
            assert (alone["step"][6400], both["step"][6400]) == ((14, 5) if v == 0.5 else (22, 9))
        if es == 2:  # the one ray the static room stops: the diagonal through the window
            assert np.nonzero(alone["count"])[0].tolist() == [6400]
    assert _cast(maps[v][0], sweep, v, min_points=3)[1]["hits"] == (6329 if v == 0.5 else 4997)


@pytest.mark.parametrize("shift", [0.0, 700.0])
@pytest.mark.parametrize("v", [0.5, 0.3])
def test_t_against_the_exact_parameter(v, shift):
    """t = fl(fl(fl(K v) - o) fl(1 / fl(P - o))) against t* = (K v - o) / (P - o) in exact rationals (K = k_a + up_a, an integer; v, o, P
    the doubles they are), u = 2^-53:
      b = fl(K v) = K v (1 + e1);  s = fl(b - o) = (b - o)(1 + e2);  d = fl(P - o) = (P - o)(1 + e3);  inv = fl(1 / d) = (1 + e4) / d;
      t = fl(s inv) = s inv (1 + e5),  |e_i| <= u
      => t = (t* + K v e1 / (P - o)) F,  F = (1 + e2)(1 + e4)(1 + e5) / (1 + e3),  |F - 1| <= 5 u  (4 u and the products of the e_i)
      => |t - t*| <= (|K v| / |P - o|) u (1 + 5 u) + 5 u |t*|
    The first term is absolute: b - o cancels, so the rounding of the product K v - relative to |b|, not to |b - o| - does not shrink with
    t.  With the rays moved 700 m from the frame's origin and a v that is no power of two (K * 0.5 is exact: e1 = 0) it is far larger than
    the second, and a bound relative in t would not hold."""
    u = Fraction(1, 2**53)
    os_, ps = _random_rays(150, 11, shift)
    chain, t, M = RR.walks_t(ps, os_, v)
    worst, worst_rel = Fraction(0), 0.0
    for r in range(len(M)):
        w = chain[: M[r] + 1, r]
        exact = RR.enter_exact(ps[r], os_[r], v, w)
        o, p = [Fraction(float(x)) for x in os_[r]], [Fraction(float(x)) for x in ps[r]]
        for i, te in enumerate(exact, start=1):
            (a,) = np.nonzero(w[i] != w[i - 1])[0]
            b = max(int(w[i][a]), int(w[i - 1][a])) * Fraction(float(v))
            bound = abs(b / (p[a] - o[a])) * u * (1 + 5 * u) + 5 * u * abs(te)
            err = abs(Fraction(float(t[i, r])) - te)
            assert err <= bound, (os_[r], ps[r], i, float(err), float(bound))
            worst = max(worst, err / bound)
            if te != 0:
                worst_rel = max(worst_rel, float(err / (abs(te) * u)))
    print("v", v, "shift", shift, "worst error / bound", float(worst), "worst error in units of u |t|", worst_rel)
    assert shift == 0.0 or v == 0.5 or worst_rel > 5.0, "the shifted rays show that the bound cannot be relative in t"


@pytest.mark.parametrize("v", [0.5, 0.3])
def test_end_shell_is_the_carves_shell(scene, v):
    """end_shell = s + 1: every hit voxel is one a carve with shell = s sees through (through >= 1), and a ray's hit is the FIRST occupied
    one among the voxels that carve counts for it"""
    sweep, _, maps = scene
    keys, cnt = maps[v][0]
    mk = CR.pack(keys)
    for s in (0, 1):
        hits, _ = _cast(maps[v][0], sweep, v, end_shell=s + 1)
        tk, tc, _, _ = CR.through_counts(sweep, CR.ROOM_ORIGIN, v, np.inf, shell=s)
        hk = CR.pack(hits["key"][hits["count"] > 0])
        assert len(hk) and np.isin(hk, tk).all()
        chain, M = CR.walks(sweep, np.broadcast_to(CR.ROOM_ORIGIN, sweep.shape), v)
        for r in range(0, len(sweep), 7):
            w = chain[: M[r] + 1, r]
            thru = w[np.abs(w - w[-1]).max(1) > s]
            occ = np.isin(CR.pack(thru), mk)
            if occ.any():
                first = int(np.argmax(occ))
                assert hits["count"][r] > 0 and hits["step"][r] == first and tuple(hits["key"][r]) == tuple(thru[first])
            else:
                assert hits["count"][r] == 0 and hits["tested"][r] == len(thru)


@pytest.mark.parametrize("fault", ["second_hit", "shell_off", "count_ignored", "t_prev", "first_off"])
def test_the_gpu_tests_checks_bite(scene, fault):
    """what test_map_raycast_gpu.py compares - every record of the room scene as bytes, for every (v, end_shell, min_points, first_step)
    of its grid - differs from the right answer for each of the five mistakes"""
    sweep, _, maps = scene
    caught = []
    for v, es, mp, fs in itertools.product((0.5, 0.3), END_SHELLS, MIN_POINTS, FIRST_STEPS):
        kw = dict(end_shell=es, min_points=mp, first_step=fs)
        good, bad = _cast(maps[v][0], sweep, v, **kw), _cast(maps[v][0], sweep, v, fault=fault, **kw)
        if good[0].tobytes() != bad[0].tobytes():
            caught.append((v, es, mp, fs))
    print(fault, "caught at", len(caught), "of 24:", caught)
    assert caught, fault
