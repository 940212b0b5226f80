"""wc_map_raycast (csrc/map.hip: k_map_raycast) and its facade surface against the numpy restatement of map_raycast_ref.py on the map's
own export(): every record of every call is compared as bytes - rays that are not cast too, no ray is left out - and the four counters as
integers.  test_map_raycast_ref.py shows that this comparison tells five mistakes from the right answer on the room scene used here.
Shapes: some 6 k rays at v >= 0.3, walks of at most about forty steps."""
import ctypes as C
import itertools

import numpy as np
import pytest

import map_carve_ref as CR
import map_raycast_ref as RR
from helpers import check_unreadable_points_refused, point_records as _records, xyz_of as _xyz
from test_map_gpu import _drive
from wildcat_slam_amd import lib
from wildcat_slam_amd import records as R
from wildcat_slam_amd import synth

pytestmark = pytest.mark.gpu

WC_ERR_ARG = 11
END_SHELLS, MIN_POINTS, FIRST_STEPS = (0, 1, 2), (1, 3), (0, 1)
BAD = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [3e38, 0, 0], [1, -3e6, 1]], np.float32)


@pytest.fixture(scope="module")
def scene():
    return CR.room_scene()


def _state(m):
    """everything a caller can read of the map without changing it"""
    return b"".join(a.tobytes() for a in m.export()), m.size(), m.info(), m.surfels().tobytes() if m.moments else b""


def _check(m, exported, pts, origin, device=None, max_range=np.inf, **kw):
    """one cast of the PointMap m held against the restatement on `exported` = m.export() -> (hits, result)"""
    cen, cnt, keys = exported
    xyz = pts if pts.dtype != R.POINT else _xyz(pts)
    want, want_res = RR.raycast(keys, cnt, cen, xyz, origin, m.voxel, max_range, **kw)
    if device is not None:
        d_hits = m.ctx.alloc(48 * max(len(xyz), 1))
        res = m.raycast_device(device, origin, lib.map_raycast_params(max_range, **kw), d_hits)
        got = d_hits.download(R.MAP_RAY_HIT, len(xyz))
        d_hits.free()
    else:
        got, res = m.raycast(pts, origin, max_range, **kw)
    what = (m.voxel, m.moments, len(xyz), kw)
    if got.tobytes() != want.tobytes():
        diff = np.nonzero([a.tobytes() != b.tobytes() for a, b in zip(got, want)])[0]
        raise AssertionError((what, len(diff), diff[:5], got[diff[:5]], want[diff[:5]]))
    assert res == want_res, (what, res, want_res)
    return got, res


@pytest.mark.parametrize("moments", [False, True])
@pytest.mark.parametrize("v", [0.5, 0.3])
def test_room_scene(gpu, scene, moments, v):
    """the map is sweep + phantom; hits at every residue of the batch length, walks of up to 24 (v = 0.5) and 40 (v = 0.3) steps"""
    sweep, phantom = scene
    assert len(sweep) == 6401 and len(phantom) == 654
    m = gpu.map_create(v, moments=moments)
    assert m.insert(np.concatenate([sweep, phantom])) == 0
    before = _state(m)
    exported = m.export()
    hits = {}
    for es, mp, fs in itertools.product(END_SHELLS, MIN_POINTS, FIRST_STEPS):
        got, res = _check(m, exported, sweep, CR.ROOM_ORIGIN, end_shell=es, min_points=mp, first_step=fs)
        hits[es, mp, fs] = res["hits"]
        assert res["rays_cast"] == len(sweep) and res["tested"] == int(got["tested"].sum())
        if (es, mp) == (0, 1):
            st = got["step"][got["count"] > 0]
            assert np.bincount(st % 8, minlength=8).min() >= 300 and st.max() == (18 if v == 0.5 else 30)
    want = {0.5: (6401, 1284, 335, 6329), 0.3: (6401, 1662, 320, 4997)}[v]  # (test_map_raycast_ref.py: the same figures without a device)
    assert (hits[0, 1, 0], hits[1, 1, 0], hits[2, 1, 0], hits[0, 3, 0]) == want
    assert _state(m) == before
    m.close()


def test_room_scene_static_map(gpu, scene):
    """a map of the sweep alone: at end_shell = 2 the static room stops exactly one ray, the diagonal through the window"""
    sweep, _ = scene
    m = gpu.map_create(0.5)
    m.insert(sweep)
    exported = m.export()
    n_hits = [_check(m, exported, sweep, CR.ROOM_ORIGIN, end_shell=es)[1]["hits"] for es in END_SHELLS]
    assert n_hits == [6401, 873, 1]
    m.close()


def test_batch_edges(gpu):
    """rays along +x from one origin, M = 0 .. 40, through a map of ONE voxel s steps from the origin, s = 0 .. 33: whatever the batch
    length up to 16, a hit at the first, the last and the middle position of a batch, at the first position of the next one, and at M
    (the ray that ends in the voxel); then the same rays through an empty map"""
    v = 0.5
    o = np.array([0.25, 0.25, 0.25])
    rays = np.stack([0.25 + 0.5 * np.arange(41), np.full(41, 0.25), np.full(41, 0.25)], -1).astype(np.float32)
    for s in range(34):
        m = gpu.map_create(v)
        m.insert(np.array([[0.25 + 0.5 * s, 0.3, 0.2]], np.float32))
        got, res = _check(m, m.export(), rays, o)
        assert res["hits"] == 41 - s and np.all(got["step"][s:] == s) and np.all(got["tested"][s:] == s + 1) and np.all(got["count"][:s] == 0)
        assert got["tested"][:s].tolist() == list(range(1, s + 1))
        if s in (1, 8, 17):  # ... and with the tested run cut at either end
            _check(m, m.export(), rays, o, first_step=s)
            _check(m, m.export(), rays, o, first_step=s + 1)
            _check(m, m.export(), rays, o, end_shell=3)
        m.close()
    e = gpu.map_create(v)
    got, res = _check(e, e.export(), rays, o)
    assert res == dict(rays_cast=41, rays_skipped=0, hits=0, tested=int(np.arange(1, 42).sum())) and np.all(np.isinf(got["t"]))
    e.close()


def test_probe_chains(gpu):
    """4096 voxels of one point each in a table of 8192 slots - as full as the growth policy lets a table be: the probe chains are long"""
    rng = np.random.Generator(np.random.PCG64(41))
    v = 0.5
    cells = rng.permutation(24**3)[:4096]
    k = np.stack([cells // 576, (cells // 24) % 24, cells % 24], -1) - 12
    pts = ((k + rng.uniform(0.1, 0.9, k.shape)) * v).astype(np.float32)
    m = gpu.map_create(v, reserve_voxels=0)
    assert m.insert(pts) == 0 and m.size() == (4096, 4096) and m.info()["slots"] == 8192
    exported = m.export()
    ends = rng.uniform(-7, 7, (1500, 3)).astype(np.float32)
    for origin in ((0.1, 0.2, 0.3), (-5.9, 5.9, 0.0), (9.0, -8.0, 7.5)):
        _, res = _check(m, exported, ends, origin)
        assert res["hits"] > 500
        _, res = _check(m, exported, ends, origin, first_step=3, end_shell=1)
        # no voxel holds two points: every tested position of every ray is probed to the end of its chain
        _, res = _check(m, exported, ends, origin, min_points=2)
        assert res["hits"] == 0 and res["tested"] > 10 * len(ends)
    m.close()


@pytest.fixture(scope="module")
def room_map(gpu, scene):
    sweep, phantom = scene
    m = gpu.map_create(0.5, moments=True)
    m.insert(np.concatenate([sweep, phantom]))
    yield m, m.export()
    m.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_layouts_and_sizes(gpu, scene, room_map, n):
    """packed xyz and 48-byte records give the same bytes, at the wavefront and workgroup edges"""
    sweep, _ = scene
    m, exported = room_map
    rays = sweep[:: max(len(sweep) // max(n, 1), 1)][:n]
    assert len(rays) == n
    a, res_a = _check(m, exported, rays, CR.ROOM_ORIGIN, end_shell=1)
    d = gpu.to_device(_records(rays)) if n else None
    b, res_b = _check(m, exported, rays, CR.ROOM_ORIGIN, device=R.Points(d.ptr if d else 0, (d.ptr + 24) if d else 0, 48, 48, n), end_shell=1)
    assert a.tobytes() == b.tobytes() and res_a == res_b and (n < 64 or res_a["hits"] > 0)
    if d:
        d.free()


def test_strided_call(gpu, scene, room_map):
    """every 10th point of the sweep through xyz_stride = 120"""
    sweep, _ = scene
    m, exported = room_map
    d = gpu.to_device(sweep)
    n = (len(sweep) + 9) // 10
    _, res = _check(m, exported, sweep[::10], CR.ROOM_ORIGIN, device=R.Points(d.ptr, 0, 120, 0, n), end_shell=2)
    assert res["rays_cast"] == n == 641 and res["hits"] > 0
    d.free()


def test_rays_not_cast(gpu):
    """NaN and inf points, keys out of range, p = o, len2 beyond either bound, M > max_steps, an origin on voxel faces, and an origin out of
    the key range, which leaves every ray uncast"""
    rng = np.random.Generator(np.random.PCG64(23))
    o = np.array([0.5, 1.0, 0.25])
    grid = (np.round(rng.uniform(-5, 5, (1500, 3)) * 4) / 4).astype(np.float32)
    special = np.array([o, o + [0.1, 0.1, 0.1], o + [3, 0, 0], o + [0, -4, 0], o + [0, 0, 2], o + [-2.5, 0, 0], o + [2, 2, 0], o + [-3, 3, 3],
                        o + [0.05, 0, 0.1], o + [9, 9, 0], o + [7.75, 0, 0], o + [0, 0.25, 0], [2e5, 0, 0], [0.3, -0.2, 0.1], [0.31, -0.21, 0.12]], np.float32)
    pts = np.concatenate([grid, special, BAD])
    fill = (np.round(rng.uniform(-5, 5, (3000, 3)) * 8) / 8).astype(np.float32)
    for v in (0.5, 0.25):
        m = gpu.map_create(v, moments=True)
        assert m.insert(np.concatenate([fill, pts])) == len(BAD)
        exported = m.export()
        for origin in (o, np.array([0.3, -0.2, 0.1]), np.array([3e6, 0.0, 0.0])):
            got, res = _check(m, exported, pts, origin, max_range=6.0, min_range=0.3, max_steps=20, end_shell=1)
            r = CR.rays(pts, origin, v, 0.3, 6.0, 20)
            if origin[0] < 1e6:
                M_all = np.abs(r["ke"] - r["k0"]).sum(1)
                assert 0 < res["rays_cast"] < len(pts) - len(BAD) and (r["end_ok"] & (M_all > 20)).any() and res["hits"] > 0
            else:
                assert res == dict(rays_cast=0, rays_skipped=len(pts), hits=0, tested=0) and np.all(got["flags"] == 1)
        m.close()


def test_determinism_and_grid_size(gpu, scene, room_map):
    sweep, _ = scene
    m, _ = room_map
    outs = []
    try:
        for groups in (0, 0, 1, 7):
            gpu.set_dev_option("map_cast_groups", groups)
            got, res = m.raycast(sweep, CR.ROOM_ORIGIN, np.inf, end_shell=1, min_points=3)
            outs.append((got.tobytes(), res))
    finally:
        gpu.set_dev_option("map_cast_groups", 0)
    assert outs[0][1]["hits"] > 0 and all(o == outs[0] for o in outs[1:])


@pytest.mark.parametrize("moments", [False, True])
def test_the_map_is_unchanged(gpu, scene, moments):
    """export, size, info (and surfels) are what they were; insert, nearest and carve behind the cast do what they do on a map that was
    never cast against"""
    sweep, phantom = scene
    v = 0.3
    pts = np.concatenate([sweep, phantom])
    m, ref = gpu.map_create(v, moments=moments), gpu.map_create(v, moments=moments)
    m.insert(pts)
    ref.insert(pts)
    before = _state(m)
    got, res = m.raycast(sweep, CR.ROOM_ORIGIN, np.inf, end_shell=2)
    assert res["hits"] == 320 and _state(m) == before == _state(ref)
    q = np.concatenate([pts[::3], BAD])
    assert m.nearest(q, v).tobytes() == ref.nearest(q, v).tobytes()
    assert m.carve(sweep, CR.ROOM_ORIGIN, np.inf, shell=1, min_rays=2) == ref.carve(sweep, CR.ROOM_ORIGIN, np.inf, shell=1, min_rays=2)
    assert m.raycast(sweep, CR.ROOM_ORIGIN, np.inf, end_shell=2)[0].tobytes() == got.tobytes()  # (the carve's scratch is its own)
    assert m.insert(sweep) == ref.insert(sweep) == 0
    assert _state(m) == _state(ref) != before
    m.close()
    ref.close()


def test_raycast_dirs(gpu, scene, room_map):
    """cast in a direction up to a reach = the cast of the float32 end points origin + reach * dir"""
    sweep, _ = scene
    m, exported = room_map
    d = sweep[::20].astype(np.float64) - CR.ROOM_ORIGIN
    rng_ = np.linalg.norm(d, axis=1)
    dirs = d / rng_[:, None]
    ends = (CR.ROOM_ORIGIN + (rng_ + 2.0)[:, None] * dirs).astype(np.float32)
    want, want_res = RR.raycast(*[exported[i] for i in (2, 1, 0)], ends, CR.ROOM_ORIGIN, m.voxel, np.inf, end_shell=0)
    got, res = m.raycast_dirs(CR.ROOM_ORIGIN, dirs, rng_ + 2.0)
    assert got.tobytes() == want.tobytes() and res == want_res and res["hits"] == len(ends)
    # every ray is stopped before its end, two metres behind the wall: the range t |end - origin| is no longer than the return's
    reach = got["t"] * np.linalg.norm(ends.astype(np.float64) - CR.ROOM_ORIGIN, axis=1)
    assert np.all(reach <= rng_ + 1e-6)


def test_argument_errors(gpu, scene, room_map):
    sweep, _ = scene
    m, exported = room_map
    before = _state(m)
    d = gpu.to_device(sweep)
    d_hits = gpu.alloc(48 * len(sweep) + 8)
    desc = R.Points(d.ptr, 0, 12, 0, len(sweep))
    o = (C.c_double * 3)(*CR.ROOM_ORIGIN)
    res = R.MapRaycastResult()
    good = lib.map_raycast_params(30.0)

    def call(ctx=gpu.h, mp=m.h, pts=C.byref(desc), org=o, par=C.byref(good), hits=C.c_void_p(d_hits.ptr), out=C.byref(res)):
        return gpu.lib.wc_map_raycast(ctx, mp, pts, org, par, hits, out)

    nan, inf = float("nan"), float("inf")
    for kw in (dict(ctx=None), dict(mp=None), dict(pts=None), dict(org=None), dict(par=None), dict(hits=None)):
        assert call(**kw) == WC_ERR_ARG, kw
    assert call(hits=C.c_void_p(d_hits.ptr + 4)) == WC_ERR_ARG  # misaligned
    for bad_o in ((nan, 0, 0), (0, inf, 0), (0, 0, -inf)):
        assert call(org=(C.c_double * 3)(*bad_o)) == WC_ERR_ARG, bad_o
    # (min_range, max_range, first_step, end_shell, min_points, max_steps)
    for fields in ((nan, 30.0, 0, 0, 1, 4096), (0.0, nan, 0, 0, 1, 4096), (-1.0, 30.0, 0, 0, 1, 4096), (0.0, -1.0, 0, 0, 1, 4096),
                   (31.0, 30.0, 0, 0, 1, 4096), (0.0, 30.0, 65537, 0, 1, 4096), (0.0, 30.0, 0, 10, 1, 4096), (0.0, 30.0, 0, 0, 0, 4096),
                   (0.0, 30.0, 0, 0, 1, 0), (0.0, 30.0, 0, 0, 1, 65537)):
        assert call(par=C.byref(R.MapRaycastParams(*fields))) == WC_ERR_ARG, fields
    assert call(pts=C.byref(R.Points(d.ptr, 0, 12, 0, 2**31))) == WC_ERR_ARG
    check_unreadable_points_refused(gpu, lambda bad: call(pts=C.byref(bad)))
    other = lib.Context(0)
    assert gpu.lib.wc_map_raycast(other.h, m.h, C.byref(desc), o, C.byref(good), C.c_void_p(d_hits.ptr), C.byref(res)) == WC_ERR_ARG
    other.close()
    assert _state(m) == before
    # n = 0 is fine without an output; the accepted ends of the ranges; an 8-aligned, not 16-aligned output
    assert call(pts=C.byref(R.Points(0, 0, 12, 0, 0)), hits=None) == 0 and (res.rays_cast, res.rays_skipped, res.hits, res.tested) == (0, 0, 0, 0)
    assert call(par=C.byref(R.MapRaycastParams(0.0, inf, 65536, 9, 1, 65536))) == 0 and call(par=C.byref(R.MapRaycastParams(5.0, 5.0, 0, 0, 2**31, 1))) == 0
    want, want_res = RR.raycast(*[exported[i] for i in (2, 1, 0)], sweep, CR.ROOM_ORIGIN, m.voxel, 30.0)
    assert call(hits=C.c_void_p(d_hits.ptr + 8)) == 0 and lib._raycast_dict(res) == want_res
    assert gpu.download_raw(d_hits.ptr + 8, 48 * len(sweep)).tobytes() == want.tobytes()
    # h_out = NULL: no wait, the same records behind the stream
    gpu.lib.wc_memset(gpu.h, C.c_void_p(d_hits.ptr), C.c_int(0xFF), C.c_size_t(48 * len(sweep)))
    assert m.raycast_device(desc, CR.ROOM_ORIGIN, good, d_hits, want_result=False) is None
    assert d_hits.download(R.MAP_RAY_HIT, len(sweep)).tobytes() == want.tobytes()
    d.free()
    d_hits.free()


def test_facade(gpu):
    """Odometry.map_raycast on the map a few facade sweeps built is PointMap.raycast on a map of the same points, and leaves the map and
    the odometry's state alone"""
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
    m = gpu.map_create(v)
    m.insert(np.concatenate(scans))
    exported = m.export()
    assert exported[0].tobytes() == xyz.tobytes() and exported[1].tobytes() == cnt.tobytes()
    samples = odo.samples().tobytes()
    rays = scans[-1][::5]
    kw = dict(min_range=0.5, end_shell=2, min_points=2)
    want, want_res = _check(m, exported, rays, origins[-1], max_range=12.0, **kw)
    got, res = odo.map_raycast(rays, origins[-1], 12.0, **kw)
    assert got.tobytes() == want.tobytes() and res == want_res and res["rays_cast"] > 0 and res["hits"] > 0
    assert odo.map_raycast(rays, origins[-1], 12.0, end_shell=10) is None  # (refused by the library)
    empty, res0 = odo.map_raycast(np.zeros((0, 3), np.float32), origins[-1], 12.0)
    assert len(empty) == 0 and res0 == dict(rays_cast=0, rays_skipped=0, hits=0, tested=0)
    xyz2, cnt2 = odo.map_export()
    assert xyz2.tobytes() == xyz.tobytes() and cnt2.tobytes() == cnt.tobytes() and odo.samples().tobytes() == samples
    odo.close()
    m.close()
    none = lib.Odometry(0)
    assert none.map_raycast(np.zeros((3, 3), np.float32), (0, 0, 0), 5.0) is None  # no map
    none.close()
