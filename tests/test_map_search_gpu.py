"""Many pose hypotheses in one pass on the device (include/wildcat_hip.h: wc_map_linearize_batch, wc_map_align_batch,
wc_map_align_pyramid_batch, wc_map_align_best, wc_pose_yaw_grid; csrc/map.hip: k_map_linearize<ONE>, k_map_lin_reduce; DESIGN
8.10): every batched call byte for byte against its single calls, the hypothesis that fails alone, the refusals, what the single and
the batched pyramid leave apart on a failing level, the yaw search on the scene of map_search_ref.py against the float64 restatement,
and the facade."""
import ctypes as C

import numpy as np
import pytest

import map_coarsen_ref as MC
import map_register_ref as G
import map_search_ref as MS
from helpers import point_records
from helpers import xyz_of as _xyz
from test_map_coarsen_gpu import new_map, summary_bytes
from test_map_gpu import _drive
from test_map_register_ref import P, scan_of
from wildcat_slam_amd import lib as L
from wildcat_slam_amd import records as R
from wildcat_slam_amd import synth

pytestmark = pytest.mark.gpu

WC_ERR_CAPACITY, WC_ERR_ARG = 1, 11
K_MAX = 64


@pytest.fixture(scope="module")
def world(gpu):
    """the room of DESIGN 8.9 at v = 0.2 and its three coarser levels (finest first); the basin scan and pose; K_MAX poses around it"""
    fine = new_map(gpu, MC.BASIN_V, True, _xyz(synth.g1_room(MC.BASIN_ROOM)))
    levels = fine.pyramid(MC.BASIN_FACTOR, MC.BASIN_LEVELS)
    T = MC.basin_pose()
    rng = np.random.default_rng(11)
    poses = np.stack([G.pose_update(T, np.concatenate([rng.normal(size=3) * 0.01, rng.normal(size=3) * 0.05])) for _ in range(K_MAX)])
    poses[0] = T
    yield dict(levels=levels, T=T, scan=scan_of(8193, T), poses=poses, kw=dict(max_iterations=MC.BASIN_ITERS, tol_rot=G.TOL_ROT, tol_trans=G.TOL_TRANS))
    for m in levels:
        m.close()


def far_pose(t):
    return np.concatenate([np.eye(3), np.full((3, 1), t)], 1)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 8193])
def test_linearize_batch_equals_the_single_calls(gpu, world, n):
    """H, g, cost and the counts - the record's 240 bytes - for K = 1, 2, 3, 33, 64 in an order that makes the scratch grow and shrink,
    both point layouts, map_lin_groups 0, 1, 7, with and without the Cauchy loss; one configuration run twice"""
    m, scan = world["levels"][1], world["scan"][:n]  # (v = 0.4: the poses' spread stays within the search)
    bufs = [gpu.to_device(scan), gpu.to_device(point_records(scan))]
    descs = [R.Points(bufs[0].ptr, 0, 12, 0, n), R.Points(bufs[1].ptr, 0, 48, 0, n)]
    try:
        for cauchy_a in (0.0, 0.4):
            prm = L.map_reg_params(m.voxel, cauchy_a=cauchy_a)
            single = np.stack([m.linearize_device(descs[0], T, prm) for T in world["poses"]])
            if n >= 255:
                assert single["n_used"].min() > n // 8 and len(set(single["cost"].tolist())) == K_MAX
            for groups in (0, 1, 7):
                gpu.set_dev_option("map_lin_groups", groups)
                for desc in descs:
                    for K in (64, 1, 33, 2, 3):
                        ne, status = m.linearize_batch_device(desc, world["poses"][:K], prm)
                        assert status.dtype == np.int32 and not status.any()
                        assert ne.tobytes() == single[:K].tobytes(), (cauchy_a, groups, desc.xyz_stride, K)
            gpu.set_dev_option("map_lin_groups", 0)
            again = m.linearize_batch_device(descs[0], world["poses"][:33], prm)[0]
            assert again.tobytes() == single[:33].tobytes()
        ne, status = m.linearize_batch(scan, world["poses"][:3], cauchy_a=0.4)  # (the uploading form)
        assert ne.tobytes() == single[:3].tobytes() and not status.any()
    finally:
        gpu.set_dev_option("map_lin_groups", 0)
        for b in bufs:
            b.free()


@pytest.mark.parametrize("n", [257, 1])
def test_linearize_with_rows_equals_the_batch_of_one(gpu, world, n):
    """wc_map_linearize with d_rows and wc_map_linearize_batch at K = 1 on the same pose: one record, for map_lin_groups 0 and 1 and both
    point layouts; the single call's rows after a batch of one and one of 33 (the scratch they share grows and shrinks) are the rows of
    the call made before them"""
    m, scan, T = world["levels"][1], world["scan"][:n], world["poses"][1]
    prm = L.map_reg_params(m.voxel, cauchy_a=0.4)
    bufs = [gpu.to_device(scan), gpu.to_device(point_records(scan))]
    d_rows = gpu.alloc(64 * n)
    try:
        for groups in (0, 1):
            gpu.set_dev_option("map_lin_groups", groups)
            for desc in (R.Points(bufs[0].ptr, 0, 12, 0, n), R.Points(bufs[1].ptr, 0, 48, 0, n)):
                ne = m.linearize_device(desc, T, prm, d_rows)
                rows = gpu.download_raw(d_rows.ptr, 64 * n).tobytes()
                assert n == 1 or (rows != bytes(64 * n) and ne["n_used"] > n // 8)
                one, status = m.linearize_batch_device(desc, T[None], prm)
                assert status.tolist() == [0] and one[0].tobytes() == ne.tobytes(), (groups, desc.xyz_stride)
                m.linearize_batch_device(desc, world["poses"][:33], prm)
                d_rows.upload(np.full(64 * n, 0x5A, np.uint8))
                again = m.linearize_device(desc, T, prm, d_rows)
                assert again.tobytes() == ne.tobytes() and gpu.download_raw(d_rows.ptr, 64 * n).tobytes() == rows, (groups, desc.xyz_stride)
    finally:
        gpu.set_dev_option("map_lin_groups", 0)
        d_rows.free()
        for b in bufs:
            b.free()


def test_one_hypothesis_of_five_fails_alone(gpu, world):
    """a translation of 1e39 sends every point to a non-finite float: that hypothesis's status is WC_ERR_ARG and its record zero, the call
    succeeds, the other four equal their single calls"""
    m, scan = world["levels"][1], world["scan"][:2000]
    prm = L.map_reg_params(m.voxel)
    Ts = world["poses"][:5].copy()
    Ts[2] = far_pose(1e39)
    ne, status = m.linearize_batch(scan, Ts, prm)
    assert status.tolist() == [0, 0, WC_ERR_ARG, 0, 0] and ne[2].tobytes() == bytes(240)
    with pytest.raises(L.WildcatError) as e:
        m.linearize(scan, Ts[2], prm)
    assert e.value.code == WC_ERR_ARG
    for h in (0, 1, 3, 4):
        assert ne[h].tobytes() == m.linearize(scan, Ts[h], prm).tobytes() and ne[h]["n_used"] > 200


def test_refusals_leave_the_outputs_untouched_and_the_empty_inputs(gpu, world):
    lib, m = gpu.lib, world["levels"][1]
    n = 1000
    d = gpu.to_device(world["scan"][:n])
    desc = R.Points(d.ptr, 0, 12, 0, n)
    prm = L.map_reg_params(m.voxel)
    good = np.ascontiguousarray(np.tile(world["T"].reshape(-1), (1025, 1)))
    out, status = np.zeros(1025, R.MAP_NORMAL_EQ), np.zeros(1025, np.int32)

    def fill():
        out.view(np.uint8)[:] = 0x5A
        status[:] = 0x5A5A5A5A

    def untouched():
        return np.all(out.view(np.uint8) == 0x5A) and np.all(status == 0x5A5A5A5A)

    def rc(ctx=gpu, mp=m, pts=desc, T=good, K=4, p=prm, o=out, s=status):
        return lib.wc_map_linearize_batch(ctx.h, mp.h if mp else None, C.byref(pts) if pts is not None else None, R.ptr(T) if T is not None else None,
                                          C.c_uint32(K), C.byref(p) if p is not None else None, R.ptr(o) if o is not None else None,
                                          R.ptr(s) if s is not None else None)

    nan_T = good[:4].copy()
    nan_T[3, 7] = np.nan
    inf_T = good[:4].copy()
    inf_T[0, 0] = np.inf
    plain = new_map(gpu, 0.25, False, world["scan"][:n])
    other = L.Context(0)
    bad_prm = L.map_reg_params(m.voxel, min_points=2)
    fill()
    cases = [dict(T=nan_T), dict(T=inf_T), dict(mp=plain), dict(ctx=other), dict(mp=None), dict(pts=None), dict(T=None), dict(p=None), dict(o=None),
             dict(s=None), dict(K=1025), dict(p=bad_prm), dict(pts=R.Points(d.ptr, 0, 8, 0, 10))]
    for kw in cases:
        assert rc(**kw) == WC_ERR_ARG and untouched(), kw
    other.close(), plain.close()
    # the capacity cap: K * ceil(n / 256) > 2^20 - a descriptor whose n alone trips it (nothing of the points is read before the check)
    assert rc(K=1, pts=R.Points(d.ptr, 0, 12, 0, 2**28 + 1)) == WC_ERR_CAPACITY and untouched()
    assert rc(K=1024, pts=R.Points(d.ptr, 0, 12, 0, 256 * 1024 + 1)) == WC_ERR_CAPACITY and untouched()
    # K = 0: nothing is touched; n = 0: zero records, every status WC_OK
    assert rc(K=0) == 0 and rc(K=0, T=None, o=None, s=None) == 0 and untouched()
    assert rc(K=4, pts=R.Points(0, 0, 12, 0, 0)) == 0
    assert out[:4].tobytes() == bytes(4 * 240) and not status[:4].any()
    assert np.all(out[4:].view(np.uint8) == 0x5A) and np.all(status[4:] == 0x5A5A5A5A)
    # the align forms refuse the same, and their own options
    Tio, summ = good[:4].copy(), (R.MapAlignSummary * 4)()
    C.memset(summ, 0x5A, C.sizeof(summ))
    summ_before, opts = bytes(summ), L.map_align_opts(prm, **world["kw"])

    def ra(mp=m, T=Tio, K=4, o=opts, pts=desc):
        return lib.wc_map_align_batch(gpu.h, mp.h, C.byref(pts), R.ptr(T), C.c_uint32(K), C.byref(o), summ, R.ptr(status))

    fill()
    for kw in (dict(T=nan_T), dict(K=1025, T=good), dict(o=L.map_align_opts(prm, max_iterations=0)), dict(o=L.map_align_opts(bad_prm)),
               dict(o=L.map_align_opts(prm, min_used=5))):
        assert ra(**kw) == WC_ERR_ARG, kw
        assert bytes(summ) == summ_before and untouched() and Tio.tobytes() == good[:4].tobytes(), kw
    assert ra(K=1, pts=R.Points(d.ptr, 0, 12, 0, 2**28 + 1)) == WC_ERR_CAPACITY and bytes(summ) == summ_before and untouched()
    handles = (C.c_void_p * 2)(world["levels"][2].h.value, m.h.value)
    two = (R.MapAlignOpts * 2)(opts, L.map_align_opts(prm, tol_rot=0.0))
    summ8 = (R.MapAlignSummary * 8)()
    C.memset(summ8, 0x5A, C.sizeof(summ8))
    assert lib.wc_map_align_pyramid_batch(gpu.h, handles, C.c_uint32(2), C.byref(desc), R.ptr(Tio), C.c_uint32(4), two, summ8,
                                          R.ptr(status)) == WC_ERR_ARG  # (the SECOND level's options: checked before the first level runs)
    assert bytes(summ8) == bytes([0x5A]) * C.sizeof(summ8) and untouched() and Tio.tobytes() == good[:4].tobytes()
    assert ra(K=0) == 0 and bytes(summ) == summ_before and untouched()
    d.free()


def align_starts(T):
    """starts that end in different rounds of one batch: the pose itself, offsets of growing size, identity (12 degrees and 0.8 m off),
    a start 500 m away (no voxel near: termination 2 in round 0) and one whose linearisation fails (status WC_ERR_ARG)"""
    rng = np.random.default_rng(3)
    near = [G.pose_update(T, np.concatenate([rng.normal(size=3) * s, rng.normal(size=3) * 4 * s])) for s in (1e-5, 1e-3, 1e-2, 3e-2)]
    return np.stack([T] + near + [np.eye(3, 4), far_pose(500.0), far_pose(1e39)])


def single_aligns(m, desc, Ts, opts):
    """K single align calls -> (poses, summaries, statuses); a refused start keeps its pose, and its summary is None"""
    out_T, out_s, out_st = [], [], []
    for T in Ts:
        Tio, summ = np.ascontiguousarray(T.reshape(-1)).copy(), R.MapAlignSummary()
        rc = m.lib.wc_map_align(m.ctx.h, m.h, C.byref(desc), R.ptr(Tio), C.byref(opts), C.byref(summ))
        out_T.append(Tio.reshape(3, 4)), out_s.append(bytes(summ)), out_st.append(rc)
    return np.stack(out_T), out_s, out_st


def test_align_batch_equals_the_single_calls(gpu, world):
    """poses, summaries (their 88 bytes) and statuses of one batch against K single wc_map_align calls - the failing start's partly filled
    summary included -, and K = 1"""
    m = world["levels"][2]  # v = 0.8
    scan = world["scan"][: MC.BASIN_SCAN]
    d = gpu.to_device(scan)
    desc = R.Points(d.ptr, 0, 12, 0, len(scan))
    opts = L.map_align_opts(L.map_reg_params(m.voxel), **world["kw"])
    starts = align_starts(world["T"])
    K = len(starts)
    T_one, s_one, st_one = single_aligns(m, desc, starts, opts)
    Tio, summ, status = np.ascontiguousarray(starts.reshape(K, 12)).copy(), (R.MapAlignSummary * K)(), np.full(K, -1, np.int32)
    assert gpu.lib.wc_map_align_batch(gpu.h, m.h, C.byref(desc), R.ptr(Tio), C.c_uint32(K), C.byref(opts), summ, R.ptr(status)) == 0
    assert status.tolist() == st_one and st_one == [0] * (K - 1) + [WC_ERR_ARG]
    assert Tio.tobytes() == T_one.tobytes()
    assert [bytes(summ[h]) for h in range(K)] == s_one
    its = [summ[h].iterations for h in range(K)]
    print("align_batch: iterations", its, "terminations", [summ[h].termination for h in range(K)])
    assert len(set(its[: K - 2])) >= 3 and summ[K - 2].termination == 2 and summ[K - 2].iterations == 0
    assert all(summ[h].termination == 0 and summ[h].n_used > 1000 for h in range(K - 3))
    # the binding's forms, and K = 1
    T_b, s_b, st_b = m.align_batch(scan, starts, opts)
    assert T_b.tobytes() == T_one.tobytes() and st_b.tolist() == st_one
    for h in (0, K - 3):
        T1, s1, st1 = m.align_batch_device(desc, starts[h : h + 1], opts)
        T_s, s_s = m.align_device(desc, starts[h], opts)
        assert T1[0].tobytes() == T_s.tobytes() == T_one[h].tobytes() and summary_bytes(s1[0]) == summary_bytes(s_s) == summary_bytes(s_b[h])
        assert st1.tolist() == [0]
    d.free()


@pytest.fixture(scope="module")
def search(gpu, world):
    """the scene of map_search_ref.py on the device: K = 8 yaw hypotheses of (I | c) through the four levels in one batched pyramid"""
    levels = world["levels"][::-1]  # coarsest first
    scan, starts = MS.search_scan(), L.pose_yaw_grid(MS.search_start(), MS.SEARCH_K)
    kw = dict(max_iterations=MS.SEARCH_ITERS, tol_rot=G.TOL_ROT, tol_trans=G.TOL_TRANS)
    Ts, summ, status = L.map_align_pyramid_batch(levels, scan, starts, **kw)
    return dict(levels=levels, scan=scan, starts=starts, kw=kw, Ts=Ts, summ=summ, status=status)


@pytest.mark.parametrize("n_levels", [1, 4])
def test_align_pyramid_batch_equals_the_single_pyramids(gpu, world, search, n_levels):
    """... for the eight yaw hypotheses and a ninth whose first linearisation fails: its status is the error, its pose stays, its later
    summaries are zero"""
    levels = search["levels"][-n_levels:]
    starts = np.concatenate([search["starts"], far_pose(1e39)[None]])
    K = len(starts)
    if n_levels == 4:  # (the fixture's run, without the ninth)
        Ts8, summ8, status8 = search["Ts"], search["summ"], search["status"]
    Ts, summ, status = L.map_align_pyramid_batch(levels, search["scan"], starts, **search["kw"])
    assert status.tolist() == [0] * (K - 1) + [WC_ERR_ARG] and Ts[K - 1].tobytes() == starts[K - 1].tobytes()
    assert len(summ) == n_levels and all(len(row) == K for row in summ)
    zero = L._summary_dict(R.MapAlignSummary())
    assert all(summary_bytes(summ[l][K - 1]) == summary_bytes(zero) for l in range(1, n_levels))
    for h in range(K - 1):
        T_s, s_s = L.map_align_pyramid(levels, search["scan"], starts[h], **search["kw"])
        assert Ts[h].tobytes() == T_s.tobytes(), h
        assert [summary_bytes(summ[l][h]) for l in range(n_levels)] == [summary_bytes(s) for s in s_s], h
    with pytest.raises(L.WildcatError):
        L.map_align_pyramid(levels, search["scan"], starts[K - 1], **search["kw"])
    if n_levels == 4:
        assert Ts8.tobytes() == Ts[:8].tobytes() and not status8.any()
        assert [[summary_bytes(s) for s in row] for row in summ8] == [[summary_bytes(s) for s in row[:8]] for row in summ]


def test_a_failing_level_ends_the_single_pyramid_and_only_the_hypothesis_of_the_batched_one(gpu, world):
    """a start whose first linearisation fails, two levels: wc_map_align_pyramid returns the error, T_io stays and the second level's
    summary is not touched; wc_map_align_pyramid_batch with K = 1 returns WC_OK with the error as the status and a ZERO second summary;
    the context then computes what it computed before"""
    lib, levels = gpu.lib, world["levels"][1::-1]  # coarsest first
    scan = world["scan"][:2000]
    d = gpu.to_device(scan)
    desc = R.Points(d.ptr, 0, 12, 0, len(scan))
    prm = L.map_reg_params(levels[1].voxel)
    before = levels[1].linearize_device(desc, world["T"], prm).tobytes()
    handles = (C.c_void_p * 2)(*[m.h.value for m in levels])
    opts = (R.MapAlignOpts * 2)(*L.map_pyramid_opts(levels, **world["kw"]))
    start = np.ascontiguousarray(far_pose(1e39).reshape(-1))
    size = C.sizeof(R.MapAlignSummary)
    Tio, summ = start.copy(), (R.MapAlignSummary * 2)()
    C.memset(summ, 0x5A, 2 * size)
    assert lib.wc_map_align_pyramid(gpu.h, handles, C.c_uint32(2), C.byref(desc), R.ptr(Tio), opts, summ) == WC_ERR_ARG
    assert Tio.tobytes() == start.tobytes() and bytes(summ[1]) == bytes([0x5A]) * size
    Tio, status = start.copy(), np.full(1, -1, np.int32)
    C.memset(summ, 0x5A, 2 * size)
    assert lib.wc_map_align_pyramid_batch(gpu.h, handles, C.c_uint32(2), C.byref(desc), R.ptr(Tio), C.c_uint32(1), opts, summ, R.ptr(status)) == 0
    assert status.tolist() == [WC_ERR_ARG] and Tio.tobytes() == start.tobytes() and bytes(summ[1]) == bytes(size)
    assert levels[1].linearize_device(desc, world["T"], prm).tobytes() == before
    d.free()


def test_yaw_search_finds_the_pose_the_pyramid_alone_loses(gpu, world, search):
    """the winner (map_align_best on the finest level) ends within twice the pose error of the restatement's winner - the float64 loop of
    map_search_ref on the levels' own exports -; hypothesis 0 is what map_align_pyramid does from this start, byte for byte, and is lost"""
    T_true, levels = MS.search_pose(), search["levels"]
    finest = search["summ"][-1]
    win = L.map_align_best(finest, search["status"], 6)
    for k, row in enumerate(MS.report(search["Ts"], finest, T_true)):
        print("search (device): k", k, "n_used", row[0], "final_cost", row[1], "termination", row[2], "error", row[3], row[4])
    assert win >= 0 and win == MS.best_ref(finest, search["status"], 6)
    surf = {m.voxel: m.surfels() for m in levels}
    Ts_ref, summ_ref = MS.search_ref(surf.get, search["scan"], search["starts"], [m.voxel for m in levels], P)
    win_ref = MS.best_ref(summ_ref[-1], [0] * MS.SEARCH_K, 6)
    e_gpu, e_ref = G.pose_error(search["Ts"][win], T_true), G.pose_error(Ts_ref[win_ref], T_true)
    print("search: device winner", win, e_gpu, "restatement's", win_ref, e_ref)
    assert win_ref >= 0 and e_ref[0] < np.deg2rad(0.1) and e_ref[1] < 0.01
    assert e_gpu[0] <= 2 * e_ref[0] and e_gpu[1] <= 2 * e_ref[1]
    T_0, _ = L.map_align_pyramid(levels, search["scan"], search["starts"][0], **search["kw"])
    assert T_0.tobytes() == search["Ts"][0].tobytes() and G.pose_error(T_0, T_true)[0] > 1.0


def test_facade(gpu):
    """Odometry.map_relocalize_search on a short room stream: n_yaw = 1 is map_relocalize byte for byte; n_yaw = 8 gives the winner of
    map_align_best over map_align_pyramid_batch on a stand-alone map fed the same published sweeps; the cases that return None"""
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
    T = np.concatenate([G.rodrigues(np.deg2rad(3.0) * np.array([0.0, 0.0, 1.0])), np.array([[0.1], [-0.2], [0.05]])], 1)
    finest = L.map_align_opts(L.map_reg_params(2 * v, 3, cauchy_a=0.4), max_iterations=6)
    size_before = odo.map_size()
    T_rel, s_rel = odo.map_relocalize(q, T, factor, n_levels, finest)
    T_one, s_one, best_one = odo.map_relocalize_search(q, T, 1, factor, n_levels, finest)
    assert best_one == 0 and T_one.tobytes() == T_rel.tobytes() and T_one.tobytes() != T.tobytes()
    assert [summary_bytes(row[0]) for row in s_one] == [summary_bytes(s) for s in s_rel]
    T_odo, s_odo, best = odo.map_relocalize_search(q, T, 8, factor, n_levels, finest)
    assert odo.map_size() == size_before
    levels = ref.pyramid(factor, n_levels)[::-1]
    opts = [L.map_align_opts(L.map_reg_params(2 * v * float(factor) ** l, 3, cauchy_a=0.4), max_iterations=6) for l in range(n_levels)][::-1]
    Ts, summ, status = L.map_align_pyramid_batch(levels, q, L.pose_yaw_grid(T, 8), opts)
    want = L.map_align_best(summ[-1], status, finest.min_used)
    assert want >= 0 and best == want and T_odo.tobytes() == Ts[want].tobytes()
    assert [[summary_bytes(s) for s in row] for row in s_odo] == [[summary_bytes(s) for s in row] for row in summ]
    for m in levels[:-1]:
        m.close()
    ref.close()
    # refused: nothing computed, no abort
    assert odo.map_relocalize_search(q, T, 0, factor, n_levels, finest) is None and odo.map_relocalize_search(q, T, 1025, factor, n_levels, finest) is None
    Tio, sentinel = np.ascontiguousarray(T.reshape(-1)).copy(), C.c_int32(77)
    for n_yaw in (0, 1025):
        assert odo.lib.wc_odom_map_relocalize_search(odo.h, R.ptr(q), C.c_uint64(len(q)), R.ptr(Tio), C.c_uint32(n_yaw), C.c_uint32(factor),
                                                     C.c_uint32(n_levels), C.byref(finest), None, C.byref(sentinel)) == 0
        assert Tio.tobytes() == T.tobytes() and sentinel.value == 77
    assert odo.map_relocalize_search(q, T, 8, factor, 9, finest) is None and odo.map_relocalize_search(q, T, 8, 7, 3, finest) is None
    odo.set_map_surfels(False)
    assert odo.map_relocalize_search(q, T, 8, factor, n_levels, finest) is None
    assert odo.lib.wc_odom_map_relocalize_search(odo.h, R.ptr(q), C.c_uint64(len(q)), R.ptr(Tio), C.c_uint32(8), C.c_uint32(factor),
                                                 C.c_uint32(n_levels), C.byref(finest), None, C.byref(sentinel)) == 0
    assert Tio.tobytes() == T.tobytes() and sentinel.value == 77
    odo.close()
