"""The voxel map's coarser levels on the device (include/wildcat_hip.h: wc_map_coarsen, wc_map_align_pyramid; csrc/map.hip:
k_map_coarsen) against the restatement of map_coarsen_ref.py: the coarsened state byte for byte, a dyadic voxel size against
the same points inserted at the coarse size, 4096 fine voxels added into one, the table's edges, tombstones, the result's later use,
the coarse-to-fine registration against its single calls and on the basin case, the refusals, and the facade."""
import ctypes as C

import numpy as np
import pytest

import map_coarsen_ref as MC
import map_query_ref as Q
import map_register_ref as G
import map_state_ref as MS
from helpers import xyz_of as _xyz
from test_map_gpu import _drive
from test_map_register_ref import P, scan_of
from wildcat_slam_amd import lib as L
from wildcat_slam_amd import records as R
from wildcat_slam_amd import synth

pytestmark = pytest.mark.gpu

WC_ERR_CAPACITY, WC_ERR_ARG = 1, 11


def new_map(gpu, v, moments, pts=None, **kw):
    m = gpu.map_create(v, moments=moments, **kw)
    if pts is not None and len(pts):
        assert m.insert(pts) == 0
    return m


def state_bytes(m):
    vox, mom = m.state()
    return vox.tobytes() + (mom.tobytes() if mom is not None else b"")


def ref_bytes(state):
    return state[0].tobytes() + (state[1].tobytes() if state[1] is not None else b"")


def summary_bytes(s):
    """every field of align's summary, exactly"""
    return np.array([s["initial_cost"], s["final_cost"]]).tobytes() + s["last_step"].tobytes() + repr(
        (s["iterations"], s["termination"], s["n_used"], s["n_found"])).encode()


def check_coarsen(src, factor, moments=None):
    """src.coarsen(factor, moments) against coarsen_ref of src's state: the state byte for byte, the counters those of the content, the
    table sized as a merge sizes an empty destination, src untouched -> the coarse map"""
    before, size_before = state_bytes(src), src.size()
    vox, mom = src.state()
    mom_out = src.moments if moments is None else moments
    want = MC.coarsen_ref(vox, mom if mom_out else None, src.voxel, factor)
    c = src.coarsen(factor, moments)
    assert c.moments == mom_out and c.voxel == MC.coarse_voxel(src.voxel, factor)
    assert state_bytes(c) == ref_bytes(want)
    assert c.size() == (len(want[0]), size_before[1])
    slots = 2
    while slots < 2 * len(vox):
        slots *= 2
    assert c.info()["slots"] == slots and c.info()["rejected"] == 0
    assert state_bytes(src) == before and src.size() == size_before
    return c


@pytest.mark.parametrize("v,factor", [(0.2, 2), (0.05, 4), (float(np.float32(0.8)) / 4, 3)])
def test_state_equals_the_restatement(gpu, v, factor):
    """moments -> moments, moments -> plain, plain -> plain, and factor 1 (a copy)"""
    xyz = _xyz(synth.g1_room(6000, seed=3))
    with_mom, plain = new_map(gpu, v, True, xyz), new_map(gpu, v, False, xyz)
    made = [check_coarsen(with_mom, factor), check_coarsen(with_mom, factor, moments=False), check_coarsen(plain, factor)]
    assert made[1].state()[1] is None and state_bytes(made[1]) == state_bytes(made[2])
    for src in (with_mom, plain):
        copy = check_coarsen(src, 1)
        assert state_bytes(copy) == state_bytes(src) and all(a.tobytes() == b.tobytes() for a, b in zip(copy.export(), src.export()))
        made.append(copy)
    for m in made + [with_mom, plain]:
        m.close()


@pytest.mark.parametrize("factor", [2, 3])
def test_dyadic_voxel_equals_the_points_inserted_at_the_coarse_size(gpu, factor):
    v = 0.25
    xyz = MC.face_cloud(4000, v, factor, seed=17 + factor)
    assert not MC.disagree(xyz, v, factor).any()
    src = new_map(gpu, v, True, xyz)
    c = check_coarsen(src, factor)
    direct = new_map(gpu, MC.coarse_voxel(v, factor), True, xyz)
    assert state_bytes(c) == state_bytes(direct) and c.size() == direct.size()
    assert c.surfels().tobytes() == direct.surfels().tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(c.export(), direct.export()))
    rng = np.random.default_rng(factor)
    q = (xyz[rng.integers(0, len(xyz), 300)] + rng.normal(size=(300, 3)) * v).astype(np.float32)
    hits = c.nearest_plane(q, np.inf)
    assert hits.tobytes() == direct.nearest_plane(q, np.inf).tobytes() and (hits["count"] != 0).sum() > 200
    for m in (src, c, direct):
        m.close()


def test_contention_4096_fine_voxels_into_one(gpu):
    """v = 0.05, factor 16: every fine voxel of coarse voxel (0, 0, 0) is filled - 4096 lanes add into one slot -, and six neighbouring
    coarse voxels hold a single fine voxel each"""
    v, factor = 0.05, 16
    rng = np.random.default_rng(4)
    k = np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), -1).reshape(-1, 3)
    centres = (k + 0.5) * v
    pts = np.concatenate([centres, centres + rng.uniform(-0.02, 0.02, centres.shape), centres[::3] + rng.uniform(-0.02, 0.02, centres[::3].shape)])
    lone = np.array([[-0.025, 0.4, 0.4], [0.825, 0.4, 0.4], [0.4, -0.025, 0.4], [0.4, 0.825, 0.4], [0.4, 0.4, -0.025], [0.4, 0.4, 0.825]])
    xyz = np.concatenate([pts, lone]).astype(np.float32)
    assert not MC.disagree(xyz, v, factor).any()
    for moments in (True, False):
        src = new_map(gpu, v, moments, xyz)
        assert src.size() == (4096 + 6, len(xyz))
        c = check_coarsen(src, factor)
        vox, _ = c.state()
        assert len(vox) == 7 and sorted(vox["count"].tolist()) == [1] * 6 + [len(pts)]
        direct = new_map(gpu, MC.coarse_voxel(v, factor), moments, xyz)
        assert state_bytes(c) == state_bytes(direct)
        for m in (src, c, direct):
            m.close()


def test_edges_empty_one_voxel_small_tables_and_negative_keys(gpu):
    for moments in (False, True):
        empty = new_map(gpu, 0.25, moments)
        c = check_coarsen(empty, 3)
        assert c.size() == (0, 0) and len(c.state()[0]) == 0 and c.info()["slots"] == 2
        assert c.insert(np.array([[0.1, 0.2, 0.3]], np.float32)) == 0 and c.size() == (1, 1)  # (an ordinary map)
        c.close(), empty.close()
        one = new_map(gpu, 0.25, moments, np.array([[-0.1, 0.3, 5.2]], np.float32), reserve_voxels=1)
        assert one.info()["slots"] == 2  # (a table smaller than a wavefront)
        c = check_coarsen(one, 3)
        assert c.state()[0]["key"].tolist() == [[-1, 0, 6]] and c.size() == (1, 1)
        c.close(), one.close()
    # tables of 256 and 512 slots: one and two workgroups, every lane a slot
    rng = np.random.default_rng(9)
    for reserve, n in ((128, 120), (256, 250)):
        xyz = rng.uniform(-3.0, 3.0, (n, 3)).astype(np.float32)
        src = new_map(gpu, 0.25, True, xyz, reserve_voxels=reserve)
        assert src.info()["slots"] == 2 * reserve and src.info()["growths"] == 0
        check_coarsen(src, 2).close()
        src.close()
    # negative keys the factor does not divide: k = -1, -factor, -factor - 1 (and their neighbours) on every axis
    v, factor = 0.25, 3
    ks = np.array([-1, -factor, -factor - 1, -factor + 1, 0, factor - 1, factor, -2 * factor - 1])
    k = np.stack(np.meshgrid(ks, ks, ks, indexing="ij"), -1).reshape(-1, 3)
    xyz = ((k + rng.uniform(0.05, 0.95, k.shape)) * v).astype(np.float32)
    src = new_map(gpu, v, True, xyz)
    assert np.array_equal(np.unique(src.state()[0]["key"]), np.sort(ks))
    c = check_coarsen(src, factor)
    assert np.array_equal(np.unique(c.state()[0]["key"]), np.unique(ks // factor)) and (ks // factor).min() == -3
    direct = new_map(gpu, MC.coarse_voxel(v, factor), True, xyz)
    assert state_bytes(c) == state_bytes(direct)
    for m in (src, c, direct):
        m.close()


def test_tombstones_are_skipped(gpu):
    v, factor = 0.25, 2
    xyz = MC.face_cloud(3000, v, factor, seed=2)
    src = new_map(gpu, v, True, xyz)
    keys = src.state()[0]["key"]
    gone = keys[::3]
    assert src.remove(gone)["voxels_removed"] == len(gone) and src.tombstones()[0] == len(gone)
    kept = ~np.isin(Q.pack(np.floor(xyz.astype(np.float64) / v).astype(np.int64)), Q.pack(gone.astype(np.int64)))
    c = check_coarsen(src, factor)
    assert ref_bytes(MS.state_of(xyz[kept], MC.coarse_voxel(v, factor))) == state_bytes(c)
    c.close()
    # a voxel that was removed and is inserted into again counts from zero
    back = ((gone[:5] + 0.5) * v).astype(np.float32)
    assert src.insert(back) == 0
    vox, _ = src.state()
    again = np.isin(Q.pack(vox["key"].astype(np.int64)), Q.pack(gone[:5].astype(np.int64)))
    assert again.sum() == 5 and np.all(vox["count"][again] == 1)
    c = check_coarsen(src, factor)
    assert ref_bytes(MS.state_of(np.concatenate([xyz[kept], back]), MC.coarse_voxel(v, factor))) == state_bytes(c)
    c.close(), src.close()


def test_the_result_grows_and_merges(gpu):
    v, factor = 0.25, 2
    V = MC.coarse_voxel(v, factor)
    a, b, far = MC.face_cloud(2000, v, factor, seed=31), MC.face_cloud(2000, v, factor, seed=32), MC.face_cloud(20_000, v, factor, seed=33, span=40.0)
    src = new_map(gpu, v, True, a)
    c = check_coarsen(src, factor)
    slots = c.info()["slots"]
    assert c.insert(far) == 0 and c.info()["slots"] > slots and c.info()["growths"] > 0
    other = new_map(gpu, V, True, b)
    c.merge(other)
    direct = new_map(gpu, V, True, np.concatenate([a, far, b]))
    assert state_bytes(c) == state_bytes(direct) and c.size() == direct.size()
    with pytest.raises(L.WildcatError):
        c.merge(src)  # (another voxel size)
    for m in (src, c, other, direct):
        m.close()


@pytest.fixture(scope="module")
def basin(gpu):
    """DESIGN 8.9's case: the room at v = 0.2 and its three coarser levels, the scan, the true pose"""
    T = MC.basin_pose()
    fine = new_map(gpu, MC.BASIN_V, True, _xyz(synth.g1_room(MC.BASIN_ROOM)))
    levels = fine.pyramid(MC.BASIN_FACTOR, MC.BASIN_LEVELS)
    assert [m.voxel for m in levels] == MC.basin_sizes() and levels[0] is fine
    kw = dict(max_iterations=MC.BASIN_ITERS, tol_rot=G.TOL_ROT, tol_trans=G.TOL_TRANS)
    yield dict(T=T, scan=scan_of(MC.BASIN_SCAN, T), levels=levels, kw=kw)
    for m in levels:
        m.close()


@pytest.mark.parametrize("n_levels", [1, 4])
def test_align_pyramid_equals_its_single_calls(gpu, basin, n_levels):
    levels = basin["levels"][:n_levels][::-1]  # coarsest first
    opts = L.map_pyramid_opts(levels, **basin["kw"])
    assert [o.reg.max_dist for o in opts] == [m.voxel for m in levels]
    d = gpu.to_device(basin["scan"])
    desc = R.Points(d.ptr, 0, 12, 0, len(basin["scan"]))
    T_pyr, s_pyr = L.map_align_pyramid_device(levels, desc, np.eye(3, 4), opts)
    T, singles = np.eye(3, 4), []
    for m, o in zip(levels, opts):
        T, s = m.align_device(desc, T, o)
        singles.append(s)
    d.free()
    assert T_pyr.tobytes() == T.tobytes() and len(s_pyr) == n_levels
    assert [summary_bytes(s) for s in s_pyr] == [summary_bytes(s) for s in singles]
    assert all(s["iterations"] >= 1 for s in s_pyr)
    T_up, s_up = L.map_align_pyramid(levels, basin["scan"], np.eye(3, 4), **basin["kw"])  # (the uploading form, default opts)
    assert T_up.tobytes() == T.tobytes() and [summary_bytes(s) for s in s_up] == [summary_bytes(s) for s in singles]


def test_basin_pyramid_recovers_where_the_fine_map_is_lost(gpu, basin):
    """from identity, 12 degrees and 0.8 m off: the four levels end within twice the restatement's pose error (the float64 loop of
    map_register_ref on the levels' own exports), the fine map alone ends more than ten times further off"""
    levels, T_true = basin["levels"][::-1], basin["T"]
    T_gpu, s_gpu = L.map_align_pyramid(levels, basin["scan"], np.eye(3, 4), **basin["kw"])
    T_fine, s_fine = basin["levels"][0].align(basin["scan"], np.eye(3, 4), params=L.map_reg_params(MC.BASIN_V), **basin["kw"])
    surf = {m.voxel: m.surfels() for m in levels}
    T_ref, s_ref = MC.basin_ref(surf.get, basin["scan"], P, [m.voxel for m in levels])
    e_gpu, e_ref, e_fine = G.pose_error(T_gpu, T_true), G.pose_error(T_ref, T_true), G.pose_error(T_fine, T_true)
    print("basin: gpu pyramid", e_gpu, [(s["iterations"], s["termination"]) for s in s_gpu], "restatement", e_ref,
          [(s["iterations"], s["termination"]) for s in s_ref], "gpu fine only", e_fine, (s_fine["iterations"], s_fine["termination"]))
    assert e_gpu[0] <= 2 * e_ref[0] and e_gpu[1] <= 2 * e_ref[1]
    assert e_ref[0] < np.deg2rad(0.1) and e_ref[1] < 0.01
    assert e_fine[0] > 10 * e_gpu[0] and e_fine[1] > 10 * e_gpu[1]


def test_refusals_leave_everything_untouched(gpu, basin):
    lib = gpu.lib
    xyz = MC.face_cloud(1000, 0.25, 2, seed=8)
    src, plain = new_map(gpu, 0.25, True, xyz), new_map(gpu, 0.25, False, xyz)
    before = state_bytes(src)
    SENTINEL = 0x5A5A5A5A
    out = C.c_void_p(SENTINEL)

    def rc(ctx=gpu, m=src, factor=2, flags=R.MAP_MOMENTS, o=out):
        return lib.wc_map_coarsen(ctx.h, m.h if m else None, C.c_uint32(factor), C.c_uint32(flags), C.byref(o) if o is not None else None)

    other = L.Context(0)
    for kw in (dict(factor=0), dict(factor=17), dict(flags=2), dict(flags=R.MAP_MOMENTS | 4), dict(m=plain), dict(m=None), dict(o=None),
               dict(ctx=other)):
        assert rc(**kw) == WC_ERR_ARG and out.value == SENTINEL, kw
    other.close()
    assert rc(factor=16) == 0 and out.value != SENTINEL  # (V = 4.0 is allowed)
    assert lib.wc_map_destroy(gpu.h, out) == 0
    # more points than one voxel may hold: a state absorbed with large counts
    big = np.zeros(3, R.MAP_VOXEL)
    big["key"], big["count"] = [[0, 0, 0], [1, 0, 0], [5, 5, 5]], 2**28
    heavy = new_map(gpu, 0.25, True)
    assert heavy.absorb(big[:2], np.zeros((2, 9), np.int64)) == 0 and heavy.size() == (2, 2**29)
    out.value = SENTINEL
    assert rc(m=heavy) == WC_ERR_CAPACITY and out.value == SENTINEL
    c = heavy.coarsen(2, moments=False)  # (2^29 <= 2^30: a plain result holds them)
    assert c.size() == (1, 2**29)
    c.close()
    heavy_plain = new_map(gpu, 0.25, False)
    big["count"] = 2**30
    assert heavy_plain.absorb(big) == 0 and heavy_plain.size() == (3, 3 * 2**30)
    assert rc(m=heavy_plain, flags=0) == WC_ERR_CAPACITY and out.value == SENTINEL
    with pytest.raises(L.WildcatError) as e:
        heavy_plain.coarsen(2)
    assert e.value.code == WC_ERR_CAPACITY
    heavy.close(), heavy_plain.close()
    # the pyramid: every level's arguments are checked before any work
    levels = basin["levels"][:2][::-1]
    good = L.map_pyramid_opts(levels, **basin["kw"])
    d = gpu.to_device(basin["scan"])
    desc = R.Points(d.ptr, 0, 12, 0, len(basin["scan"]))
    T0 = np.ascontiguousarray(np.eye(3, 4).reshape(-1))
    T, summ = T0.copy(), (R.MapAlignSummary * 9)()
    C.memset(summ, 0x5A, C.sizeof(summ))
    summ_before = bytes(summ)

    def rp(ctx=gpu, maps=levels, n=None, opts=good, pts=desc, Tio=T, s=summ):
        n = len(maps) if n is None else n
        h = (C.c_void_p * max(len(maps), 1))(*[m.h.value if m else None for m in maps])
        return lib.wc_map_align_pyramid(ctx.h, h, C.c_uint32(n), C.byref(pts) if pts is not None else None, R.ptr(Tio) if Tio is not None else None,
                                        (R.MapAlignOpts * max(len(opts), 1))(*opts) if opts is not None else None, s)

    def bad_opts(**kw):
        o = L.map_pyramid_opts(levels, **basin["kw"])
        for f, x in kw.items():
            setattr(o[1].reg if f in ("max_dist", "min_points", "reserved", "sigma0", "cauchy_a") else o[1], f, x)
        return o

    other = L.Context(0)
    nan_T = T0.copy()
    nan_T[7] = np.nan
    cases = [dict(n=0), dict(maps=levels * 5, opts=good * 5, n=9), dict(maps=[levels[0], plain]), dict(maps=[levels[0], None]), dict(ctx=other),
             dict(pts=None), dict(Tio=None), dict(opts=None), dict(s=None), dict(Tio=nan_T), dict(pts=R.Points(d.ptr, 0, 8, 0, 10))]
    cases += [dict(opts=bad_opts(**kw)) for kw in (dict(reserved=1), dict(max_dist=0.0), dict(min_points=2), dict(sigma0=0.0), dict(cauchy_a=-1.0),
                                                   dict(max_iterations=0), dict(tol_rot=0.0), dict(tol_trans=np.nan), dict(min_used=5),
                                                   dict(min_pivot=0.0))]
    for kw in cases:
        assert rp(**kw) == WC_ERR_ARG, kw
        assert T.tobytes() == T0.tobytes() and bytes(summ) == summ_before, kw
    other.close()
    assert rp(maps=levels * 4, opts=good * 4) == 0 and T.tobytes() != T0.tobytes()  # (8 levels, unrelated to one another, are allowed)
    d.free()
    # ... and the context still computes what it computed before
    assert state_bytes(src) == before
    check_coarsen(src, 2).close()
    src.close(), plain.close()


def test_facade(gpu):
    """Odometry.map_relocalize on a short room stream equals pyramid() + map_align_pyramid on a stand-alone map fed the same published
    sweeps, byte for byte; the cases that return None"""
    msgs, imu, _ = synth.raw_stream(1.7, pts_per_s=300_000, gyro_bias=(0.0, 0.0, 0.02), t_start=1000.0)
    v, factor, n_levels = 0.1, 2, 3
    odo = L.Odometry(0)
    odo.set_fill_outputs(True)
    odo.set_map_voxel(v)
    odo.set_map_surfels(True)
    scans = []
    _drive(odo, msgs, imu, lambda: scans.append(_xyz(odo.outputs()["scan"])))
    assert odo.sweeps() >= 2
    ref = new_map(gpu, v, True)
    for s in scans:
        assert ref.insert(s) == 0
    q = scans[-1][::3]
    w = np.deg2rad(3.0) * np.array([0.0, 0.0, 1.0])
    T = np.concatenate([G.rodrigues(w), np.array([[0.1], [-0.2], [0.05]])], 1)
    finest = L.map_align_opts(L.map_reg_params(2 * v, 3, cauchy_a=0.4), max_iterations=6)
    size_before = odo.map_size()
    T_odo, s_odo = odo.map_relocalize(q, T, factor, n_levels, finest)
    assert odo.map_size() == size_before
    levels = ref.pyramid(factor, n_levels)[::-1]
    opts = [L.map_align_opts(L.map_reg_params(2 * v * float(factor) ** l, 3, cauchy_a=0.4), max_iterations=6) for l in range(n_levels)][::-1]
    T_ref, s_ref = L.map_align_pyramid(levels, q, T, opts)
    assert T_odo.tobytes() == T_ref.tobytes() and T_odo.tobytes() != T.tobytes()
    assert [summary_bytes(s) for s in s_odo] == [summary_bytes(s) for s in s_ref] and len(s_odo) == n_levels
    assert all(s["iterations"] >= 1 for s in s_odo) and s_odo[0]["n_used"] > 100
    # one level is AlignToMap
    T_one, s_one = odo.map_relocalize(q, T, factor, 1, finest)
    T_al, s_al = odo.map_align(q, T, finest)
    assert T_one.tobytes() == T_al.tobytes() and summary_bytes(s_one[0]) == summary_bytes(s_al)
    # refused: nothing computed, no abort
    assert odo.map_relocalize(q, T, factor, 0, finest) is None and odo.map_relocalize(q, T, factor, 9, finest) is None
    assert odo.map_relocalize(q, T, 0, 2, finest) is None
    assert odo.map_relocalize(q, T, 7, 3, finest) is None  # (0.1 x 49 > 4.0)
    assert odo.map_relocalize(q, T, factor, n_levels, L.map_align_opts(L.map_reg_params(v, 2))) is None
    assert odo.map_relocalize(q, T, factor, n_levels, finest)[0].tobytes() == T_ref.tobytes()
    for m in levels:
        m.close()
    odo.set_map_surfels(False)
    assert odo.map_relocalize(q, T, factor, n_levels, finest) is None
    odo.set_map_voxel(0.0)
    assert odo.map_relocalize(q, T, factor, n_levels, finest) is None
    odo.close()
