"""wc_map_carve (csrc/map.hip: k_map_carve and the word-predicate forms of the crop's count and rehash) and its facade surface against
the numpy restatement of map_carve_ref.py.  This version of the call selects and counts, it does not remove: the five counters - rays
used and skipped, steps, and the voxels and points the rays select on the map's own export - are the restatement's, over a grid of shell
and min_rays that tells a wrong walk from the right one (test_map_carve_ref.py), and export(), surfels(), size() and info() are what
they were before the call.  Shapes: some 20 k rays at v >= 0.25, walks of at most about a hundred steps."""
import ctypes as C

import numpy as np
import pytest

import map_carve_ref as CR
import map_query_ref as Q
from helpers import check_unreadable_points_refused, point_records as _records, xyz_of as _xyz
from test_map_gpu import _drive
from wildcat_slam_amd import lib
from wildcat_slam_amd import records as R
from wildcat_slam_amd import synth

pytestmark = pytest.mark.gpu

WC_ERR_ARG = 11
SHELLS, MIN_RAYS = (0, 1, 2), (1, 2, 5)
BAD = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [3e38, 0, 0], [1, -3e6, 1]], np.float32)


@pytest.fixture(scope="module")
def room():
    """the room cloud of the other map tests as ONE sweep from the sensor's position in the middle of it -> (sweep, extra, origin); extra:
    what the map holds besides the sweep - a second sweep of the room with other range noise (wall voxels this sweep has no return in), a
    phantom blob 3.6 m from the sensor and a phantom trail that runs out to 20 m, where a voxel is crossed by a ray or two"""
    sweep = _xyz(synth.g1_room(20_000))
    origin = synth.traj_pos(0.25) + np.array([0.0, 0.0, 1.5])
    rng = np.random.Generator(np.random.PCG64(17))
    blob = origin + np.array([3.0, 2.0, 0.0]) + 0.6 * rng.uniform(-1, 1, (400, 3))
    trail = origin + np.array([-1.0, 3.0, 0.0]) + rng.uniform(0, 1, (600, 1)) * np.array([-17.0, 9.0, 1.0]) + 0.3 * rng.uniform(-1, 1, (600, 3))
    extra = np.concatenate([blob.astype(np.float32), trail.astype(np.float32), _xyz(synth.g1_room(20_000, seed=99))])  # (the blob first)
    return sweep, extra, origin


_through = {}


def _pre(tag, pts, origin, v, max_range, min_range, shell, max_steps):
    """through_counts() once per (points, origin, v, ranges, shell, max_steps): min_rays and the map do not enter it"""
    key = (tag, v, max_range, min_range, shell, max_steps)
    if key not in _through:
        _through[key] = CR.through_counts(pts, origin, v, max_range, min_range, shell, max_steps)
    return _through[key]


def _carve_and_check(m, pts, origin, tag=None, device=None, max_range=np.inf, min_range=0.0, shell=1, min_rays=1, max_steps=4096):
    """one carve of the PointMap m held against the restatement on m's own export -> (keep, result)"""
    v = m.voxel
    xyz = pts if pts.dtype != R.POINT else _xyz(pts)
    cen, cnt, keys = m.export()
    sur = m.surfels() if m.moments else None
    info = m.info()
    pre = _pre(tag, xyz, origin, v, max_range, min_range, shell, max_steps) if tag else None
    keep, want = CR.carve(keys, cnt, xyz, origin, v, max_range, min_range, shell, min_rays, max_steps, pre=pre)
    if device is not None:
        got = m.carve_device(device, origin, lib.map_carve_params(max_range, min_range, shell, min_rays, max_steps))
    else:
        got = m.carve(pts, origin, max_range, min_range, shell, min_rays, max_steps)
    what = (v, m.moments, shell, min_rays, len(xyz))
    assert got == want, (what, got, want)
    # the map is as it was
    assert all(a.tobytes() == b.tobytes() for a, b in zip(m.export(), (cen, cnt, keys))), what
    if m.moments:
        assert m.surfels().tobytes() == sur.tobytes(), what
    assert m.size() == (len(cnt), int(cnt.astype(np.int64).sum())) and m.info() == info, what
    return keep, want


@pytest.mark.parametrize("moments", [False, True])
@pytest.mark.parametrize("v", [0.5, 0.3])
def test_room_scene(gpu, room, moments, v):
    sweep, extra, origin = room
    blob = np.unique(CR.point_keys(extra[:400], v), axis=0)
    removed = {}
    for shell in SHELLS:
        for min_rays in MIN_RAYS + (len(sweep) + 1,):
            m = gpu.map_create(v, moments=moments)
            assert m.insert(np.concatenate([sweep, extra])) == 0
            keep, res = _carve_and_check(m, sweep, origin, tag="room", shell=shell, min_rays=min_rays)
            removed[shell, min_rays] = res["voxels_removed"]
            if min_rays > len(sweep):
                assert keep.all() and res["voxels_removed"] == 0
            if min_rays == 1 and shell == 1:  # the blob is selected, but for voxels next to a return
                left = np.isin(CR.pack(blob), CR.pack(m.export()[2][keep]))
                ends = np.unique(CR.point_keys(sweep, v), axis=0)
                assert all(np.abs(ends - k).max(1).min() <= 1 for k in blob[left]) and left.sum() < len(blob) // 4
            m.close()
    # the scene tells the parameters apart: fewer voxels go with a larger shell and with a larger min_rays
    for shell in SHELLS:
        assert removed[shell, 1] > removed[shell, 2] > removed[shell, 5] > 0
    for min_rays in MIN_RAYS:
        assert removed[0, min_rays] > removed[1, min_rays] > removed[2, min_rays]


def test_scene_with_exact_ties(gpu):
    """the scene of test_map_carve_ref.py: a dyadic origin, a ray whose every step is a tie at v = 0.5"""
    sweep, extra = CR.room_scene()
    for v in (0.5, 0.3):
        for shell in SHELLS:
            for min_rays in MIN_RAYS:
                m = gpu.map_create(v)
                m.insert(np.concatenate([sweep, extra]))
                _carve_and_check(m, sweep, CR.ROOM_ORIGIN, tag="ties", shell=shell, min_rays=min_rays)
                m.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_layouts_and_sizes(gpu, room, n):
    """48-byte records and packed xyz give the same bytes and counters; a strided call equals the call on the subsampled array"""
    sweep, extra, origin = room
    rays = sweep[:: len(sweep) // n][:n]
    assert len(rays) == n
    outs = []
    for layout in ("xyz12", "point48", "strided"):
        m = gpu.map_create(0.5, moments=True)
        m.insert(np.concatenate([sweep, extra]))
        if layout == "xyz12":
            keep, res = _carve_and_check(m, rays, origin, shell=1, min_rays=1)
            assert n < 64 or res["voxels_removed"] > 0
        elif layout == "point48":
            d = gpu.to_device(_records(rays))
            keep, res = _carve_and_check(m, rays, origin, device=R.Points(d.ptr, d.ptr + 24, 48, 48, n), shell=1, min_rays=1)
            d.free()
        else:  # every third row of an array three times as long
            wide = np.full((3 * n, 3), np.nan, np.float32)
            wide[::3] = rays
            d = gpu.to_device(wide)
            keep, res = _carve_and_check(m, rays, origin, device=R.Points(d.ptr, 0, 36, 0, n), shell=1, min_rays=1)
            d.free()
        outs.append((m.export(), m.surfels(), res))
        m.close()
    for o in outs[1:]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(o[0], outs[0][0])) and o[1].tobytes() == outs[0][1].tobytes() and o[2] == outs[0][2]


def test_skipped_and_degenerate_rays(gpu):
    """NaN and inf points, keys out of range, p = o, M = 0, len2 beyond either bound, M > max_steps, an origin on voxel faces, axis-parallel
    rays, and 3000 rays between points of the 0.25 m grid (exact ties and faces at v = 0.5 and 0.25)"""
    rng = np.random.Generator(np.random.PCG64(23))
    o = np.array([0.5, 1.0, 0.25])
    grid = (np.round(rng.uniform(-5, 5, (3000, 3)) * 4) / 4).astype(np.float32)
    special = np.array([o, o + [0.1, 0.1, 0.1], o + [3, 0, 0], o + [0, -4, 0], o + [0, 0, 2], o + [-2.5, 0, 0], o + [2, 2, 0], o + [-3, 3, 3],
                        o + [0.05, 0, 0.1], o + [9, 9, 0], o + [7.75, 0, 0], o + [0, 0.25, 0], [2e5, 0, 0], [0.3, -0.2, 0.1], [0.31, -0.21, 0.12]], np.float32)
    pts = np.concatenate([grid, special, BAD])
    fill = (np.round(rng.uniform(-5, 5, (6000, 3)) * 8) / 8).astype(np.float32)  # the map: occupied voxels all over the volume
    for v in (0.5, 0.25):
        for origin in (o, np.array([0.3, -0.2, 0.1]), np.array([3e6, 0.0, 0.0])):
            for shell, min_rays in ((0, 1), (1, 2)):
                m = gpu.map_create(v, moments=True)
                assert m.insert(np.concatenate([fill, pts])) == len(BAD)
                keep, res = _carve_and_check(m, pts, origin, tag=("deg", tuple(origin)), max_range=6.0, min_range=0.3, shell=shell,
                                             min_rays=min_rays, max_steps=20)
                r = CR.rays(pts, origin, v, 0.3, 6.0, 20)
                if origin[0] < 1e6:
                    assert 0 < res["rays_used"] < len(pts) - len(BAD) and res["voxels_removed"] > 0
                    M_all = np.abs(r["ke"] - r["k0"]).sum(1)
                    assert (r["end_ok"] & (M_all > 20)).any() and (r["end_ok"] & (M_all == 0)).any()
                else:
                    assert res["rays_used"] == 0 and res["rays_skipped"] == len(pts) and keep.all()
                m.close()


def test_determinism_and_grid_size(gpu, room):
    sweep, extra, origin = room
    outs = []
    try:
        for groups in (0, 0, 1, 7):
            gpu.set_dev_option("map_carve_groups", groups)
            m = gpu.map_create(0.3, moments=True)
            m.insert(np.concatenate([sweep, extra]))
            res = m.carve(sweep, origin, np.inf, shell=1, min_rays=2)
            outs.append((b"".join(a.tobytes() for a in m.export()), m.surfels().tobytes(), res, m.info()))
            m.close()
    finally:
        gpu.set_dev_option("map_carve_groups", 0)
    assert outs[0][2]["voxels_removed"] > 0 and all(o == outs[0] for o in outs[1:])


def test_after_the_carve(gpu, room):
    """the map is untouched and usable: a second call gives the same counters; wc_map_nearest is the query restatement on the export;
    the sweep inserted again gives the map of all the points"""
    sweep, extra, origin = room
    v = 0.3
    pts = np.concatenate([sweep, extra])
    m = gpu.map_create(v)
    m.insert(pts)
    _, res = _carve_and_check(m, sweep, origin, tag="room", shell=1, min_rays=2)
    assert res["voxels_removed"] > 0 and m.carve(sweep, origin, np.inf, shell=1, min_rays=2) == res
    cen, cnt, keys = m.export()
    q = np.concatenate([pts, BAD])
    want, idx = Q.nearest_voxel(keys, cen, cnt, q, v, v)
    assert 0 < (idx >= 0).sum() < len(q) and m.nearest(q, v).tobytes() == want.tobytes()
    assert m.insert(sweep) == 0
    ref = gpu.map_create(v)
    ref.insert(np.concatenate([pts, sweep]))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(m.export(), ref.export())) and m.size() == ref.size()
    m.close()
    ref.close()


def test_empty_inputs(gpu, room):
    sweep, extra, origin = room
    zero = dict(rays_used=0, rays_skipped=0, steps=0, voxels_removed=0, points_removed=0)
    e = gpu.map_create(0.5)
    _carve_and_check(e, sweep[:1000], origin, shell=1, min_rays=1)  # an empty map: the ray counters are still the restatement's
    assert e.size() == (0, 0) and e.carve(np.zeros((0, 3), np.float32), origin, np.inf) == zero
    e.close()
    m = gpu.map_create(0.5)
    m.insert(sweep)
    before = m.export()
    assert m.carve(np.zeros((0, 3), np.float32), origin, np.inf) == zero
    assert all(a.tobytes() == b.tobytes() for a, b in zip(m.export(), before))
    m.close()


def test_argument_errors(gpu, room):
    sweep, extra, origin = room
    m = gpu.map_create(0.5, moments=True)
    m.insert(np.concatenate([sweep, extra]))
    before, sur, info = m.export(), m.surfels(), m.info()
    d = gpu.to_device(sweep)
    desc = R.Points(d.ptr, 0, 12, 0, len(sweep))
    o = (C.c_double * 3)(*origin)
    res = R.MapCarveResult()
    good = lib.map_carve_params(30.0)

    def call(ctx=gpu.h, mp=m.h, pts=C.byref(desc), org=o, par=C.byref(good), out=C.byref(res)):
        return gpu.lib.wc_map_carve(ctx, mp, pts, org, par, out)

    nan, inf = float("nan"), float("inf")
    for kw in (dict(ctx=None), dict(mp=None), dict(pts=None), dict(org=None), dict(par=None), dict(out=None)):
        assert call(**kw) == WC_ERR_ARG, kw
    for bad_o in ((nan, 0, 0), (0, inf, 0), (0, 0, -inf)):
        assert call(org=(C.c_double * 3)(*bad_o)) == WC_ERR_ARG, bad_o
    for fields in ((nan, 30.0, 1, 1, 4096, 0), (0.0, nan, 1, 1, 4096, 0), (-1.0, 30.0, 1, 1, 4096, 0), (0.0, -1.0, 1, 1, 4096, 0),
                   (31.0, 30.0, 1, 1, 4096, 0), (0.0, 30.0, 9, 1, 4096, 0), (0.0, 30.0, 1, 0, 4096, 0), (0.0, 30.0, 1, 1, 0, 0),
                   (0.0, 30.0, 1, 1, 65537, 0), (0.0, 30.0, 1, 1, 4096, 1)):
        assert call(par=C.byref(R.MapCarveParams(*fields))) == WC_ERR_ARG, fields
    assert call(pts=C.byref(R.Points(d.ptr, 0, 12, 0, 2**31))) == WC_ERR_ARG
    check_unreadable_points_refused(gpu, lambda bad: call(pts=C.byref(bad)))
    other = lib.Context(0)
    assert gpu.lib.wc_map_carve(other.h, m.h, C.byref(desc), o, C.byref(good), C.byref(res)) == WC_ERR_ARG
    other.close()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(m.export(), before)) and m.surfels().tobytes() == sur.tobytes() and m.info() == info
    # the accepted ends of the ranges: max_range = +inf, min_range = max_range, shell 8, max_steps 65536
    assert call(par=C.byref(R.MapCarveParams(0.0, inf, 8, 1, 65536, 0))) == 0 and call(par=C.byref(R.MapCarveParams(5.0, 5.0, 0, 1, 1, 0))) == 0
    d.free()
    m.close()


def test_facade(gpu):
    """Odometry.map_carve on the map a few facade sweeps built is the restatement on its export, and leaves the map and the odometry's
    state alone"""
    msgs, imu, _ = synth.raw_stream(1.7, pts_per_s=300_000, gyro_bias=(0.0, 0.0, 0.02), t_start=1000.0)
    v = 0.5
    odo = lib.Odometry(0)
    odo.set_fill_outputs(True)
    odo.set_map_voxel(v)
    scans, origins = [], []

    def on_sweep():
        out = odo.outputs()
        scans.append(_xyz(out["scan"]))
        origins.append(np.asarray(out["tf"][1:4], np.float64))

    _drive(odo, msgs, imu, on_sweep)
    assert odo.sweeps() >= 2
    xyz, cnt = odo.map_export()
    keys, ref_cnt = CR.voxels_of(np.concatenate(scans), v)
    assert np.array_equal(cnt, ref_cnt)
    samples = odo.samples().tobytes()
    rays = scans[-1][::5]
    keep, want = CR.carve(keys, ref_cnt, rays, origins[-1], v, 12.0, 0.5, shell=1, min_rays=1, max_steps=4096)
    assert odo.map_carve(rays, origins[-1], 12.0, 0.5, shell=1, min_rays=1, max_steps=4096) == want and want["voxels_removed"] > 0
    assert odo.map_carve(rays, origins[-1], 12.0, shell=9) is None  # (refused by the library)
    xyz2, cnt2 = odo.map_export()
    assert xyz2.tobytes() == xyz.tobytes() and cnt2.tobytes() == cnt.tobytes() and odo.samples().tobytes() == samples
    odo.close()
    none = lib.Odometry(0)
    assert none.map_carve(np.zeros((3, 3), np.float32), (0, 0, 0), 5.0) is None  # no map
    none.close()
