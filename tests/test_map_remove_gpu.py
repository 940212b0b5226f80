"""Removal in place (csrc/map.hip: the tombstone, k_map_erase, k_map_remove_keys, the room policy of csrc/map_room.h).

The yardstick throughout is fresh-map equivalence: after a removal the map must be indistinguishable, through every call that reads it,
from a fresh map of the points whose voxel was not removed (map_remove_ref.Survivors keeps those points).  Every output of the map is
defined independently of the table's layout, so every comparison below is of bytes or integers.  Shapes: tables of 8192 and 16384 slots,
the 7055-point room scene of map_carve_ref.py, a few thousand queries."""
import ctypes as C

import numpy as np
import pytest

import map_carve_ref as CR
import map_remove_ref as MR
from helpers import check_unreadable_points_refused, xyz_of as _xyz
from map_query_ref import pack
from test_map_gpu import _drive
from wildcat_slam_amd import lib
from wildcat_slam_amd import records as R
from wildcat_slam_amd import synth

pytestmark = pytest.mark.gpu

WC_ERR_ARG = 11
V = MR.CLUSTER_V
SLOTS = MR.CLUSTER_SLOTS
RESERVE = SLOTS // 2


def _bytes(parts):
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts if p is not None)


def _same(a, b, queries, rays, origin, what=""):
    """every call that reads a map gives the same bytes on a and b"""
    assert a.size() == b.size(), what
    assert _bytes(a.export()) == _bytes(b.export()), what
    assert _bytes(a.state()) == _bytes(b.state()), what
    assert a.nearest(queries, a.voxel).tobytes() == b.nearest(queries, b.voxel).tobytes(), what
    ha, ra = a.raycast(rays, origin, np.inf)
    hb, rb = b.raycast(rays, origin, np.inf)
    assert ha.tobytes() == hb.tobytes() and ra == rb, what
    assert a.carve(rays, origin, np.inf, shell=1, min_rays=1) == b.carve(rays, origin, np.inf, shell=1, min_rays=1), what
    if a.moments:
        assert a.surfels().tobytes() == b.surfels().tobytes(), what
        assert a.nearest_plane(queries, a.voxel).tobytes() == b.nearest_plane(queries, b.voxel).tobytes(), what
        (na, rwa), (nb, rwb) = (m.linearize(queries, np.eye(3, 4), want_rows=True, max_dist=2 * m.voxel) for m in (a, b))
        assert na.tobytes() == nb.tobytes() and rwa.tobytes() == rwb.tobytes(), what


def _fresh(gpu, ref, moments, reserve=0):
    """the map of the surviving points"""
    m = gpu.map_create(ref.v, reserve_voxels=reserve, moments=moments)
    if len(ref.points):
        assert m.insert(ref.points) == 0
    return m


def _check(gpu, m, ref, rays, origin, what=""):
    """m against the fresh map of ref's points, and against the restatement's voxel list"""
    keys, cnt = ref.voxels()
    got = m.export()
    assert np.array_equal(got[2], keys) and np.array_equal(got[1], cnt), what
    f = _fresh(gpu, ref, m.moments)
    pts = ref.points
    queries = np.concatenate([pts[:: max(len(pts) // 3000, 1)], rays[:: max(len(rays) // 1000, 1)]]) if len(pts) else rays[:1000]
    _same(m, f, queries, rays, origin, what)
    f.close()


def _random_rays(seed, n, lo, hi):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.uniform(lo, hi, (n, 3)).astype(np.float32)


# ---- the cluster -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("moments", [False, True])
def test_cluster(gpu, moments):
    """a 64-key collision cluster in an 8192-slot table that is exactly half full: every second key of the cluster and a random half of
    the rest go; the chains through the tombstones still find what is behind them; re-inserted voxels start from zero; the re-insert is
    a purge (test_map_remove_ref.py runs the same scenario on the table model with each fault)"""
    sc = MR.cluster_scenario()
    first = np.concatenate([sc["cluster"], sc["rest"]])
    assert len(first) == RESERVE
    m, ref = gpu.map_create(V, reserve_voxels=RESERVE, moments=moments), MR.Survivors(V)
    pts = MR.centre_points(first)
    assert m.insert(pts) == 0
    ref.insert(pts)
    assert m.info()["slots"] == SLOTS and m.info()["growths"] == 0 and m.tombstones() == (0, 0)
    # queries: every voxel's own point (the removed ones' included) and points beside them; rays through the dense block
    queries = np.concatenate([pts, pts + np.float32(0.25), MR.centre_points(sc["fresh"])])
    rays, origin = _random_rays(5, 2000, -20.0, 20.0), np.array([0.1, 0.2, 0.3])
    want = ref.remove(sc["remove_list"])
    assert want["voxels_removed"] == len(sc["removed"]) == want["points_removed"] and want["keys_unused"] == len(sc["remove_list"]) - len(sc["removed"])
    assert m.remove(sc["remove_list"]) == want
    assert m.tombstones() == (len(sc["removed"]), 0) and m.info()["slots"] == SLOTS and m.info()["growths"] == 0
    assert m.size() == (RESERVE - len(sc["removed"]),) * 2
    f = _fresh(gpu, ref, moments)
    _same(m, f, queries, rays, origin, "removed")
    f.close()
    # a third of the removed voxels again, with other points (two each), and voxels the map never held
    more = np.concatenate([MR.centre_points(sc["again"], 0.125), MR.centre_points(sc["again"], 0.375), MR.centre_points(sc["fresh"], 0.125)])
    assert m.insert(more) == 0
    ref.insert(more)
    # 2 (live + tombstones + points) > 8192 >= 2 (live + points): a purge
    assert m.tombstones() == (0, 1) and m.info()["slots"] == SLOTS and m.info()["growths"] == 0
    f = _fresh(gpu, ref, moments)
    _same(m, f, queries, rays, origin, "inserted again")
    keys, cnt = ref.voxels()
    again = np.isin(pack(keys), pack(sc["again"]))
    assert again.sum() == len(sc["again"]) and np.all(m.export()[1][again] == 2)  # (from zero: the first life's point is not counted)
    f.close()
    m.close()


# ---- purge and growth ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("moments", [False, True])
@pytest.mark.parametrize("n_new, slots, purges", [(1200, SLOTS, 1), (5000, 2 * SLOTS, 0)])
def test_purge_and_growth(gpu, moments, n_new, slots, purges):
    """3000 voxels, 2500 removed, then n_new points in new voxels: 2 (500 + 2500 + 1200) = 8400 > 8192 >= 2 (500 + 1200) is a purge into a
    fresh table of the same size; 2 (500 + 5000) > 8192 is a growth to 16384 slots.  Either replacement drops the tombstones"""
    rng = np.random.Generator(np.random.PCG64(31))
    keys = MR.distinct_keys(rng, 3000 + 5000, -30, 30)
    old, new = keys[:3000], keys[3000 : 3000 + n_new]
    m, ref = gpu.map_create(V, reserve_voxels=RESERVE, moments=moments), MR.Survivors(V)
    assert m.insert(MR.centre_points(old)) == 0  # (asking for the rejected count waits: the occupied count is exact from here on)
    ref.insert(MR.centre_points(old))
    gone = old[rng.permutation(3000)[:2500]]
    assert m.remove(gone) == ref.remove(gone) == dict(voxels_removed=2500, points_removed=2500, keys_unused=0)
    assert m.tombstones() == (2500, 0) and m.info()["slots"] == SLOTS and m.size() == (500, 500)
    assert m.insert(MR.centre_points(new, 0.125)) == 0
    ref.insert(MR.centre_points(new, 0.125))
    info = m.info()
    assert info["slots"] == slots and info["growths"] == (0 if purges else 1) and m.tombstones() == (0, purges)
    rays = _random_rays(6, 2000, -15.0, 15.0)
    _check(gpu, m, ref, rays, np.array([0.1, 0.2, 0.3]), (n_new, moments))
    m.close()


# ---- the room scene --------------------------------------------------------------------------------------------------------------
SHELLS, MIN_RAYS = (0, 1, 2), (1, 2)
FIGURES = {
    0.5: {(0, 1): (46, 652), (0, 2): (44, 650), (1, 1): (28, 452), (1, 2): (26, 450), (2, 1): (15, 357), (2, 2): (14, 356)},
    0.3: {(0, 1): (144, 650), (0, 2): (144, 650), (1, 1): (89, 450), (1, 2): (89, 450), (2, 1): (47, 332), (2, 2): (38, 306)},
}


@pytest.fixture(scope="module")
def scene():
    sweep, phantom = CR.room_scene()
    return sweep, phantom, np.concatenate([sweep, phantom])


@pytest.mark.parametrize("moments", [False, True])
@pytest.mark.parametrize("v", [0.5, 0.3])
def test_room_scene(gpu, scene, moments, v):
    sweep, phantom, both = scene
    o = CR.ROOM_ORIGIN
    for shell in SHELLS:
        for min_rays in MIN_RAYS:
            what = (v, moments, shell, min_rays)
            m, ref = gpu.map_create(v, moments=moments), MR.Survivors(v)
            assert m.insert(both) == 0
            ref.insert(both)
            before, state_before = m.export(), m.state()
            keep, want = CR.carve(before[2], before[1], sweep, o, v, np.inf, shell=shell, min_rays=min_rays)
            assert (want["voxels_removed"], want["points_removed"]) == FIGURES[v][shell, min_rays], what
            assert m.carve_remove(sweep, o, np.inf, shell=shell, min_rays=min_rays) == want, what
            assert ref.carve_remove(sweep, o, np.inf, shell=shell, min_rays=min_rays)[0] == want
            assert m.tombstones() == (want["voxels_removed"], 0), what
            # the export and the state afterwards are those before, filtered by the restatement's keep
            assert _bytes(m.export()) == _bytes(p[keep] for p in before), what
            assert _bytes(m.state()) == _bytes(p[keep] if p is not None else None for p in state_before), what
            assert m.size() == (int(keep.sum()), int(before[1][keep].astype(np.int64).sum())), what
            # the counting call on the carved map is the restatement on its export; a second removal takes nothing
            after = m.export()
            _, zero = CR.carve(after[2], after[1], sweep, o, v, np.inf, shell=shell, min_rays=min_rays)
            assert zero["voxels_removed"] == 0 and all(zero[k] == want[k] for k in ("rays_used", "rays_skipped", "steps"))
            assert m.carve(sweep, o, np.inf, shell=shell, min_rays=min_rays) == zero, what
            assert m.carve_remove(sweep, o, np.inf, shell=shell, min_rays=min_rays) == zero and m.tombstones() == (want["voxels_removed"], 0), what
            if shell == 1:
                _check(gpu, m, ref, sweep, o, what)
            # the phantom again: the map of the survivors plus the phantom
            assert m.insert(phantom) == 0
            ref.insert(phantom)
            f = _fresh(gpu, ref, moments)
            assert _bytes(m.export()) == _bytes(f.export()) and _bytes(m.state()) == _bytes(f.state()) and m.size() == f.size(), what
            f.close()
            m.close()


# ---- other calls behind a removal ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("moments", [False, True])
def test_merge_absorb_and_crop_behind_a_removal(gpu, scene, moments):
    sweep, phantom, both = scene
    v, o = 0.3, CR.ROOM_ORIGIN
    other = _xyz(synth.g1_room(5000, seed=5))

    def carved():
        m, ref = gpu.map_create(v, moments=moments), MR.Survivors(v)
        m.insert(both)
        ref.insert(both)
        res = m.carve_remove(sweep, o, np.inf, shell=1, min_rays=1)
        assert res == ref.carve_remove(sweep, o, np.inf, shell=1, min_rays=1)[0] and res["voxels_removed"] == 89
        return m, ref

    # a carved source into a fresh destination; a fresh source into a carved destination
    src, ref = carved()
    dst = gpu.map_create(v, moments=moments)
    dst.insert(other)
    dst.merge(src)
    ref.insert(other)
    _check(gpu, dst, ref, sweep, o, "merge: carved src")
    dst.close()
    src.close()
    dst, ref = carved()
    src = gpu.map_create(v, moments=moments)
    src.insert(np.concatenate([other, phantom]))
    dst.merge(src)
    ref.insert(np.concatenate([other, phantom]))
    _check(gpu, dst, ref, sweep, o, "merge: carved dst")
    src.close()
    dst.close()
    # the state of a carved map into an empty map
    m, ref = carved()
    vox, mom = m.state()
    e = gpu.map_create(v, moments=moments)
    assert e.absorb(vox, mom) == 0
    _check(gpu, e, ref, sweep, o, "absorb")
    e.close()
    # a crop of a carved map: the replacement drops the tombstones
    lo, hi = np.array([-2.0, -3.5, -1.0]), np.array([4.5, 1.0, 2.0])
    keys, _ = ref.voxels()
    k = np.asarray(keys, np.float64)
    kept = np.all((k >= np.floor(lo / v)) & (k <= np.floor(hi / v)), axis=1)
    assert 0 < kept.sum() < len(kept) and m.tombstones() == (89, 0)
    assert m.crop(lo, hi) == int((~kept).sum())
    ref.remove(np.asarray(keys)[~kept])
    assert m.tombstones() == (0, 0)
    _check(gpu, m, ref, sweep, o, "crop")
    m.close()


# ---- edges -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 256, 257])
def test_key_counts_and_grid_sizes(gpu, n):
    """n keys - present, absent, out of range, duplicates - with one workgroup, seven, and the default grid, and twice: the same bytes"""
    rng = np.random.Generator(np.random.PCG64(100 + n))
    keys = MR.distinct_keys(rng, 600, -6, 6)
    pts = np.concatenate([MR.centre_points(keys), MR.centre_points(keys[:200], 0.125)])
    cand = np.concatenate([keys[:300], keys[:40], MR.distinct_keys(rng, 40, 50, 60), [[MR.KEY_LIM, 0, 0], [0, 0, -MR.KEY_LIM]]]).astype(np.int32)
    rm = cand[rng.permutation(len(cand))[:n]]
    outs = []
    try:
        for groups in (0, 0, 1, 7):
            gpu.set_dev_option("map_remove_groups", groups)
            m, ref = gpu.map_create(V, moments=True), MR.Survivors(V)
            m.insert(pts)
            ref.insert(pts)
            want = ref.remove(rm)
            assert m.remove(rm) == want and sum(want[k] for k in ("voxels_removed", "keys_unused")) == n
            assert m.tombstones() == (want["voxels_removed"], 0)
            if groups == 1:
                _check(gpu, m, ref, _random_rays(7, 500, -3.0, 3.0), np.array([0.1, 0.2, 0.3]), n)
            outs.append((_bytes(m.export()), _bytes(m.state()), m.size(), m.info()))
            m.close()
    finally:
        gpu.set_dev_option("map_remove_groups", 0)
    assert all(o == outs[0] for o in outs[1:])


def test_everything_removed_and_an_empty_map(gpu, scene):
    sweep, phantom, both = scene
    v, o = 0.5, CR.ROOM_ORIGIN
    m, ref = gpu.map_create(v, moments=True), MR.Survivors(v)
    m.insert(both)
    ref.insert(both)
    keys = m.export()[2]
    want = ref.remove(keys)
    assert m.remove(keys) == want == dict(voxels_removed=len(keys), points_removed=len(both), keys_unused=0)
    assert m.size() == (0, 0) and all(len(p) == 0 for p in m.export()) and len(m.state()[0]) == 0 and len(m.surfels()) == 0
    assert m.tombstones() == (len(keys), 0)
    assert m.remove(keys[:100]) == dict(voxels_removed=0, points_removed=0, keys_unused=100)
    hits, res = m.raycast(sweep, o, np.inf)
    assert res["hits"] == 0 and not hits["count"].any()
    assert m.insert(sweep) == 0  # an insert afterwards works, and finds the voxels again
    ref.insert(sweep)
    _check(gpu, m, ref, sweep, o, "inserted after everything went")
    m.close()
    # a map that never held anything
    e, eref = gpu.map_create(v), MR.Survivors(v)
    assert e.remove(keys[:10]) == dict(voxels_removed=0, points_removed=0, keys_unused=10)
    assert e.remove(np.zeros((0, 3), np.int32)) == dict(voxels_removed=0, points_removed=0, keys_unused=0)
    assert e.carve_remove(sweep[:1000], o, np.inf) == eref.carve_remove(sweep[:1000], o, np.inf)[0]
    zero = dict(rays_used=0, rays_skipped=0, steps=0, voxels_removed=0, points_removed=0)
    assert e.carve_remove(np.zeros((0, 3), np.float32), o, np.inf) == zero
    assert e.size() == (0, 0) and e.tombstones() == (0, 0)
    e.close()


def test_argument_errors(gpu, scene):
    sweep, phantom, both = scene
    m = gpu.map_create(0.5, moments=True)
    m.insert(both)

    def snapshot():
        return _bytes(m.export()), _bytes(m.state()), m.info(), m.size(), m.tombstones()

    before = snapshot()
    d = gpu.to_device(sweep)
    desc = R.Points(d.ptr, 0, 12, 0, len(sweep))
    o = (C.c_double * 3)(*CR.ROOM_ORIGIN)
    res = R.MapCarveResult()
    good = lib.map_carve_params(30.0)

    def carve(ctx=gpu.h, mp=m.h, pts=C.byref(desc), org=o, par=C.byref(good), out=C.byref(res)):
        return gpu.lib.wc_map_carve_remove(ctx, mp, pts, org, par, out)

    nan, inf = float("nan"), float("inf")
    for kw in (dict(ctx=None), dict(mp=None), dict(pts=None), dict(org=None), dict(par=None), dict(out=None)):
        assert carve(**kw) == WC_ERR_ARG, kw
    for bad_o in ((nan, 0, 0), (0, inf, 0), (0, 0, -inf)):
        assert carve(org=(C.c_double * 3)(*bad_o)) == WC_ERR_ARG, bad_o
    for fields in ((nan, 30.0, 1, 1, 4096, 0), (0.0, nan, 1, 1, 4096, 0), (-1.0, 30.0, 1, 1, 4096, 0), (0.0, -1.0, 1, 1, 4096, 0),
                   (31.0, 30.0, 1, 1, 4096, 0), (0.0, 30.0, 9, 1, 4096, 0), (0.0, 30.0, 1, 0, 4096, 0), (0.0, 30.0, 1, 1, 0, 0),
                   (0.0, 30.0, 1, 1, 65537, 0), (0.0, 30.0, 1, 1, 4096, 1)):  # (the last: reserved = 1)
        assert carve(par=C.byref(R.MapCarveParams(*fields))) == WC_ERR_ARG, fields
    assert carve(pts=C.byref(R.Points(d.ptr, 0, 12, 0, 2**31))) == WC_ERR_ARG
    check_unreadable_points_refused(gpu, lambda bad: carve(pts=C.byref(bad)))

    keys = np.ascontiguousarray(m.export()[2][:64], np.int32)
    dk = gpu.to_device(keys)
    out3 = (C.c_uint64 * 3)()

    def remove(ctx=gpu.h, mp=m.h, ptr=dk.ptr, n=64, out=out3):
        return gpu.lib.wc_map_remove_keys(ctx, mp, C.c_void_p(ptr), C.c_uint64(n), out)

    for kw in (dict(ctx=None), dict(mp=None), dict(ptr=0), dict(out=None), dict(ptr=dk.ptr + 2), dict(ptr=dk.ptr + 1), dict(n=2**31 + 1)):
        assert remove(**kw) == WC_ERR_ARG, kw
    out2 = (C.c_uint64 * 2)()
    assert gpu.lib.wc_map_tombstones(gpu.h, m.h, None) == WC_ERR_ARG and gpu.lib.wc_map_tombstones(gpu.h, None, out2) == WC_ERR_ARG
    other = lib.Context(0)
    assert gpu.lib.wc_map_carve_remove(other.h, m.h, C.byref(desc), o, C.byref(good), C.byref(res)) == WC_ERR_ARG
    assert gpu.lib.wc_map_remove_keys(other.h, m.h, C.c_void_p(dk.ptr), C.c_uint64(64), out3) == WC_ERR_ARG
    assert gpu.lib.wc_map_tombstones(other.h, m.h, out2) == WC_ERR_ARG
    other.close()
    assert snapshot() == before
    # n = 0 looks at no pointer; the accepted ends of the carve's ranges
    assert remove(ptr=0, n=0) == 0 and list(out3) == [0, 0, 0] and snapshot() == before
    assert carve(par=C.byref(R.MapCarveParams(5.0, 5.0, 0, 1, 1, 0))) == 0 and carve(par=C.byref(R.MapCarveParams(0.0, inf, 8, 1, 65536, 0))) == 0
    dk.free()
    d.free()
    m.close()


# ---- the facade ------------------------------------------------------------------------------------------------------------------
def test_facade(gpu):
    """Odometry.set_map_carve: after every sweep's insert the sweep's own rays take what they contradict; the final map is the sequential
    restatement - per sweep insert, CR.carve with that sweep's scan and origin, drop what it selects - and not the map without the option"""
    msgs, imu, _ = synth.raw_stream(1.7, pts_per_s=300_000, gyro_bias=(0.0, 0.0, 0.02), t_start=1000.0)
    v = 0.5
    runs = {}
    for on in (False, True):
        odo = lib.Odometry(0)
        odo.set_fill_outputs(True)
        odo.set_map_voxel(v)
        for bad in ((-1.0, 1, 1), (float("nan"), 1, 1), (12.0, 9, 1), (12.0, 1, 0)):
            with pytest.raises(lib.WildcatError):
                odo.set_map_carve(*bad)
        if on:
            odo.set_map_carve(12.0, 1, 1)
        scans, origins, ms = [], [], []

        def on_sweep():
            out = odo.outputs()
            scans.append(_xyz(out["scan"]))
            origins.append(np.asarray(out["tf"][1:4], np.float64))
            ms.append(odo.map_ms())

        _drive(odo, msgs, imu, on_sweep)
        assert odo.sweeps() >= 2 and all(t > 0 for t in ms)
        runs[on] = (odo.map_export(), scans, origins)
        if on:
            ref, taken = MR.Survivors(v), 0
            for scan, origin in zip(scans, origins):
                ref.insert(scan)
                taken += ref.carve_remove(scan, origin, 12.0, shell=1, min_rays=1)[0]["voxels_removed"]
            assert taken > 0
            f = _fresh(gpu, ref, False)
            xyz, cnt, _ = f.export()
            assert odo.map_export()[0].tobytes() == xyz.tobytes() and odo.map_export()[1].tobytes() == cnt.tobytes()
            assert odo.map_size()[:2] == f.size()
            # the two removal calls on the facade's map
            rays = scans[0][::3]
            want = ref.carve_remove(rays, origins[-1], 20.0, 0.5, shell=0, min_rays=1)[0]
            assert odo.map_carve(rays, origins[-1], 20.0, 0.5, shell=0, min_rays=1) == want and want["voxels_removed"] > 0
            assert odo.map_carve_remove(rays, origins[-1], 20.0, 0.5, shell=0, min_rays=1) == want
            assert odo.map_carve_remove(rays, origins[-1], 20.0, shell=9) is None  # (refused by the library)
            keys = np.concatenate([ref.voxels()[0][::7], [[MR.KEY_LIM, 0, 0]]]).astype(np.int32)
            assert odo.map_remove(keys) == ref.remove(keys)
            assert odo.map_remove(np.zeros((0, 3), np.int32)) == dict(voxels_removed=0, points_removed=0, keys_unused=0)
            f.close()
            f = _fresh(gpu, ref, False)
            xyz, cnt, _ = f.export()
            assert odo.map_export()[0].tobytes() == xyz.tobytes() and odo.map_export()[1].tobytes() == cnt.tobytes()
            f.close()
        odo.close()
    (off_xyz, off_cnt), off_scans, _ = runs[False]
    (on_xyz, on_cnt), on_scans, _ = runs[True]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(off_scans, on_scans))  # the option leaves the odometry alone ...
    assert len(on_cnt) < len(off_cnt)  # ... and did something to the map
    none = lib.Odometry(0)
    assert none.map_carve_remove(np.zeros((3, 3), np.float32), (0, 0, 0), 5.0) is None and none.map_remove(np.zeros((3, 3), np.int32)) is None
    none.close()
