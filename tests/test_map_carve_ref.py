"""The restatement of wc_map_carve (map_carve_ref.py) on its own, without a GPU: hand-worked walks, the walk's invariants on random
rays, the float walk against the walk in exact rationals, the carving of a room scene, and a demonstration that the comparisons the GPU
test makes (the five counters over its grid of shell and min_rays) tell a wrong walk from the right one."""
import itertools

import numpy as np
import pytest

import map_carve_ref as CR

V = 0.5
O = (0.25, 0.25, 0.25)


def test_hand_cases():
    assert CR.walk((3.25, 0.25, 0.25), O, V) == [(x, 0, 0) for x in range(7)]
    # the crossings of x = 0.5 and y = 0.5 coincide exactly (t = 0.25 on both axes): the lowest axis goes first, every time
    assert CR.walk((1.25, 1.25, 0.25), O, V) == [(0, 0, 0), (1, 0, 0), (1, 1, 0), (2, 1, 0), (2, 2, 0)]
    assert CR.walk_exact((1.25, 1.25, 0.25), O, V) == ([(0, 0, 0), (1, 0, 0), (1, 1, 0), (2, 1, 0), (2, 2, 0)], True)
    # inside one voxel, and p = o: M = 0
    assert CR.walk((0.4, 0.1, 0.3), O, V) == [(0, 0, 0)] and CR.walk(O, O, V) == [(0, 0, 0)]
    r = CR.rays(np.array([O, (0.4, 0.1, 0.3)], np.float32), O, V, 0.0, np.inf, 1)
    assert r["M"].tolist() == [0, 0] and r["used"].all()
    # zero direction components: along -y, and in the xz plane
    assert CR.walk((0.25, -1.25, 0.25), O, V) == [(0, 0, 0), (0, -1, 0), (0, -2, 0), (0, -3, 0)]
    w = CR.walk((1.25, 0.25, -0.75), O, V)
    assert w[0] == (0, 0, 0) and w[-1] == (2, 0, -2) and all(k[1] == 0 for k in w) and len(w) == 5
    # an origin exactly on a voxel face (x = 0.5 belongs to voxel 1): up, the first face is x = 1.0; down, it is x = 0.5 at t = 0
    assert CR.walk((1.75, 0.25, 0.25), (0.5, 0.25, 0.25), V) == [(1, 0, 0), (2, 0, 0), (3, 0, 0)]
    assert CR.walk((-0.75, 0.25, 0.25), (0.5, 0.25, 0.25), V) == [(1, 0, 0), (0, 0, 0), (-1, 0, 0), (-2, 0, 0)]
    assert CR.walk((0.25, 0.75, 0.25), (0.5, 0.5, 0.5), V) == [(1, 1, 1), (0, 1, 1), (0, 1, 0)]


def test_used_rays_and_counters_by_hand():
    pts = np.array([(3.25, 0.25, 0.25), (np.nan, 0, 0), (0, np.inf, 0), (3e6, 0, 0), (0.25, 0.25, 0.25), (0.25, 2.25, 0.25), (0.25, 9.25, 0.25)],
                   np.float32)
    r = CR.rays(pts, O, V, 1.0, 5.0, 5)
    # finite and in range: 0, 4, 5, 6; p = o is nearer than min_range; (0.25, 9.25, 0.25) is beyond max_range; ray 0 has M = 6 > 5
    assert r["end_ok"].tolist() == [True, False, False, False, True, True, True]
    assert r["used"].tolist() == [False, False, False, False, False, True, False] and r["M"].tolist() == [0, 0, 0, 0, 0, 4, 0]
    keys = np.array([(0, 0, 0), (0, 1, 0), (0, 2, 0), (0, 3, 0), (0, 4, 0), (6, 0, 0)])
    keep, res = CR.carve(keys, np.arange(1, 7), pts, O, V, 5.0, 1.0, shell=1, min_rays=1, max_steps=5)
    # ray 5 sees through (0, 0..2, 0) at shell 1; (0, 0, 0) is the end voxel of point 4, (6, 0, 0) of the skipped ray 0
    assert keep.tolist() == [True, False, False, True, True, True]
    assert res == dict(rays_used=1, rays_skipped=6, steps=4, voxels_removed=2, points_removed=5)
    # range bounds are inclusive on the squares: len2 = 4.0 exactly
    assert CR.rays(pts[5:6], O, V, 2.0, 2.0, 4)["used"].all() and not CR.rays(pts[5:6], O, V, 2.0, 2.0, 3)["used"].any()
    # an origin out of the key range: nothing is used, the end marks stay
    far = CR.rays(pts, (3e6, 0, 0), V, 0.0, np.inf, 65536)
    assert not far["used"].any() and far["end_ok"].sum() == 4


def test_shell_filter():
    pts = np.array([(3.25, 0.25, 0.25)], np.float32)
    for shell, want in ((0, range(0, 6)), (1, range(0, 5)), (2, range(0, 4))):
        tk, tc, ek, _ = CR.through_counts(pts, O, V, np.inf, shell=shell)
        assert tk.tolist() == CR.pack([(x, 0, 0) for x in want]).tolist() and np.all(tc == 1) and ek.tolist() == CR.pack([(6, 0, 0)]).tolist()
    # Chebyshev: a diagonal ray's voxel is inside the shell when EVERY axis is within it
    w = CR.walk((2.25, 2.25, 0.25), O, V)
    tk, _, _, _ = CR.through_counts(np.array([(2.25, 2.25, 0.25)], np.float32), O, V, np.inf, shell=1)
    assert sorted(tk.tolist()) == sorted(CR.pack([k for k in w if max(abs(k[0] - 4), abs(k[1] - 4), abs(k[2])) > 1]).tolist())


def _random_rays(n, seed, v):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.uniform(-1, 1, (n, 3)), rng.uniform(-8, 8, (n, 3)).astype(np.float32)


@pytest.mark.parametrize("v", [0.5, 0.25, 0.3])
def test_walk_properties(v):
    """every walk is a 6-connected chain of exactly M + 1 distinct voxels from k0 to ke; reversing the sign of an axis mirrors it"""
    os_, ps = _random_rays(1000, 5, v)
    chain, M = CR.walks(ps, os_, v)
    k0, ke = np.floor(os_ / v).astype(np.int64), np.floor(ps.astype(np.float64) / v).astype(np.int64)
    assert np.array_equal(chain[0], k0) and np.array_equal(chain[M, np.arange(len(M))], ke) and len(chain) == M.max() + 1
    mirrors = []
    for a in range(3):
        s = np.ones(3)
        s[a] = -1.0
        mirrors.append(CR.walks(ps * s.astype(np.float32), os_ * s, v)[0])
    for r in range(len(M)):
        w = chain[: M[r] + 1, r]
        assert np.all(np.abs(np.diff(w, axis=0)).sum(1) == 1) and len(np.unique(w, axis=0)) == len(w)
        for a in range(3):
            # the mirror image of voxel k on axis a is -1 - k (no coordinate of a random ray lies on a face)
            back = mirrors[a][: M[r] + 1, r].copy()
            back[:, a] = -1 - back[:, a]
            assert np.array_equal(back, w), (os_[r], ps[r], a)


@pytest.mark.parametrize("v", [0.5, 0.25, 0.3])
def test_float_walk_against_the_exact_walk(v):
    """3000 random rays: the float walk is the exact walk; a ray may be left out only when two of its exact candidate parameters at some
    step differ by at most 2^-48 relative, and fewer than 1 % may be"""
    os_, ps = _random_rays(3000, 1, v)
    chain, M = CR.walks(ps, os_, v)
    left_out = 0
    for r, (o, p) in enumerate(zip(os_, ps)):
        e, near = CR.walk_exact(p, o, v)
        if near:
            left_out += 1
            continue
        assert [tuple(k) for k in chain[: M[r] + 1, r].tolist()] == e, (o, p, v)
    print("v =", v, "left out", left_out, "of 3000")
    assert left_out < 30


def test_vectorised_walk_is_the_single_walk():
    os_, ps = _random_rays(200, 9, 0.3)
    o = os_[0]
    tk, tc, ek, r = CR.through_counts(ps, o, 0.3, np.inf, shell=0)
    want = {}
    for p in ps:
        w = CR.walk(p, o, 0.3)
        for k in w[:-1]:
            want[int(CR.pack([k])[0])] = want.get(int(CR.pack([k])[0]), 0) + 1
    assert dict(zip(tk.tolist(), tc.tolist())) == want and r["M"].sum() == sum(len(CR.walk(p, o, 0.3)) - 1 for p in ps)


SHELLS, MIN_RAYS = (0, 1, 2), (1, 2, 5)


@pytest.fixture(scope="module")
def scene():
    sweep, phantom = CR.room_scene()
    out = {}
    for v in (0.5, 0.3):
        keys, cnt = CR.voxels_of(np.concatenate([sweep, phantom]), v)
        out[v] = (keys, cnt)
    return sweep, phantom, out


@pytest.mark.parametrize("v", [0.5, 0.3])
def test_room_scene(scene, v):
    """min_rays = 1, shell = 1: every phantom voxel inside the room farther than the shell from every return's voxel goes, no voxel holding
    a return does; of the four phantom points beside the window ray's diagonal, outside the room, the x-first walk takes its two"""
    sweep, phantom, maps = scene
    keys, cnt = maps[v]
    keep, res = CR.carve(keys, cnt, sweep, CR.ROOM_ORIGIN, v, np.inf, shell=1, min_rays=1)
    mk = CR.pack(keys)
    has_return = np.isin(mk, CR.pack(CR.point_keys(sweep, v)))
    assert keep[has_return].all()
    pk = CR.point_keys(phantom, v)
    sk = np.unique(CR.point_keys(sweep, v), axis=0)
    inside = np.all((phantom > CR.ROOM_LO) & (phantom < CR.ROOM_HI), axis=1)
    assert (~inside).sum() == 4
    far = inside & np.array([np.abs(sk - k).max(1).min() > 1 for k in pk])
    assert far.sum() > 100, "the scene has phantom points in free space"
    assert not keep[np.searchsorted(mk, CR.pack(pk[far]))].any()
    if v == 0.5:
        assert keep[np.searchsorted(mk, CR.pack(pk[~inside]))].tolist() == [False, True, False, True]
    assert res["rays_used"] == len(sweep) and res["rays_skipped"] == 0 and res["voxels_removed"] == int((~keep).sum()) > 0
    assert res["points_removed"] == int(cnt[~keep].sum()) and res["steps"] > len(sweep)


@pytest.mark.parametrize("fault", ["stop_early", "tie_high", "shell_off", "twice"])
def test_the_gpu_tests_checks_bite(scene, fault):
    """what test_map_carve_gpu.py compares - the five counters, the selected voxels and their points among them, for every
    (v, shell, min_rays) of its grid - differs from the right answer for each of the four mistakes"""
    sweep, phantom, maps = scene
    caught = []
    for v, shell, min_rays in itertools.product((0.5, 0.3), SHELLS, MIN_RAYS):
        keys, cnt = maps[v]
        good = CR.carve(keys, cnt, sweep, CR.ROOM_ORIGIN, v, np.inf, shell=shell, min_rays=min_rays)
        bad = CR.carve(keys, cnt, sweep, CR.ROOM_ORIGIN, v, np.inf, shell=shell, min_rays=min_rays, fault=fault)
        if not np.array_equal(good[0], bad[0]) or good[1] != bad[1]:
            caught.append((v, shell, min_rays))
    print(fault, "caught at", caught)
    assert caught, fault
