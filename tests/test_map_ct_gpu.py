"""Continuous-time registration against the voxel map on the device (wc_map_linearize_ct, wc_map_align_ct, csrc/map.hip:
k_map_linearize_ct, k_map_lin_reduce<80, 76>) against the restatement of map_ct_ref.py on the map's own export: rows and moved points
byte for byte, the 76 sums within the bound their additions allow and byte-equal to the stated order, determinism over grids, layouts and
outputs, the stamp edges, the moved points as a map, the Gauss-Newton loop digit for digit, the prior, the refused arguments and the
facade."""
import ctypes as C

import numpy as np
import pytest

import map_ct_ref as CT
import map_register_ref as G
from extract_ref import LD
from helpers import check_unreadable_points_refused, xyz_of as _xyz
from test_map_ct_ref import TB, TE, begin_pose, end_pose, start_poses, sweep_of
from test_map_gpu import _drive
from test_map_register_gpu import COST_ROUNDINGS, LOG1P_EPS
from test_map_register_ref import P
from wildcat_slam_amd import lib as L
from wildcat_slam_amd import records as R
from wildcat_slam_amd import synth

pytestmark = pytest.mark.gpu

EPS = G.EPS
VS = float(np.float32(0.8))
WC_ERR_ARG = 11
N_SCAN = 256 * 33 + 7  # 34 tiles: a second stage with more than 32 partials, a ragged last tile


def _params(p):
    return L.map_reg_params(p.max_dist, p.min_points, p.sigma0, p.cauchy_a)


def _bytes(x):
    return np.asarray(x).tobytes()


@pytest.fixture(scope="module")
def world(gpu):
    """the maps (g1_room at v = 0.2 and 0.8f) with their exports, the two true poses and the sweep measured between them"""
    room = _xyz(synth.g1_room(200_000))
    maps = {}
    for v in (0.2, VS):
        m = gpu.map_create(v, moments=True)
        assert m.insert(room) == 0
        maps[v] = (m, m.surfels())
    pb, pe = begin_pose(), end_pose()
    body, times = sweep_of(N_SCAN + 200, pb, pe)
    assert len(body) >= N_SCAN
    yield dict(maps=maps, pb=pb, pe=pe, body=body[:N_SCAN].copy(), times=times[:N_SCAN].copy())
    for m, _ in maps.values():
        m.close()


def _descs(gpu, body, times):
    """both layouts of a stamped sweep -> [(name, buffers, wc_points)]"""
    n = len(body)
    d12, d8, d48 = gpu.to_device(body), gpu.to_device(times), gpu.to_device(synth.make_points(body, times))
    return [("xyz12 + t8", (d12, d8), R.Points(d12.ptr, d8.ptr, 12, 8, n)), ("point48", (d48,), R.Points(d48.ptr, d48.ptr + 24, 48, 48, n))]


def _free(descs):
    for _, bufs, _ in descs:
        for b in bufs:
            b.free()


def _check_sums(ne, ref, n, loss, what):
    """|gpu - ref| <= (A(n) + 6) 2^-53 sum |term| on each of the 75 weighted sums: a term ((k a) a J_i) J_j carries five roundings
    (map_ct_ref.TERM_ROUNDINGS: the weight products add three to wc_map_linearize's two), its way into the sum at most A(n) additions - the
    order is wc_map_linearize's -, and one more 2^-53 covers the second-order terms and the reference's own longdouble roundings.  cost: as
    test_map_register_gpu derives it"""
    A = G.adds_bound(n)
    worst = 0.0
    for name, _ in CT.NAMES:
        err = np.abs(ne[name].astype(LD) - ref[name])
        bound = (A + CT.SUM_C) * EPS * ref["abs" + name]
        worst = max(worst, float(np.max(err / np.where(bound > 0, bound, 1))))
        assert np.all(err <= bound), (what, name, err, bound)
    roundings = COST_ROUNDINGS + LOG1P_EPS if loss else 2
    err, bound = abs(LD(ne["cost"]) - ref["cost"]), (A + roundings + 1) * EPS * ref["abscost"]
    print(what, "A(n) =", A, "max |gpu - ref| / bound =", worst, "cost:", float(err / bound) if bound > 0 else 0.0)
    assert err <= bound, (what, "cost", err, bound)


@pytest.mark.parametrize("v", [0.2, VS])
def test_rows_and_moved_points_are_the_restatement_byte_for_byte(gpu, world, v):
    """the Cauchy loss off and on, both point layouts: d_rows and d_xyz_out equal the restatement byte for byte, the counts equal its own,
    the bytes behind the n records are untouched, and the sums meet their bound"""
    m, surf = world["maps"][v]
    body, times, pb, pe, n = world["body"], world["times"], world["pb"], world["pe"], N_SCAN
    descs = _descs(gpu, body, times)
    d_rows, d_xyz = gpu.alloc(72 * (n + 4)), gpu.alloc(12 * (n + 4))
    for cauchy_a in (0.0, 0.4):
        prm = P(v, cauchy_a=cauchy_a)
        want = CT.rows_ct(surf, body, times, pb, pe, TB, TE, v, prm)
        ref = CT.normal_eq_ct(want["rows"], want["w2"], cauchy_a)
        assert want["n_used"] > 1000 and want["n_outside"] == 0
        for name, _, desc in descs:
            tag = (v, cauchy_a, name)
            d_rows.upload(np.full(18 * (n + 4), 0xA5A5A5A5, np.uint32))
            d_xyz.upload(np.full(3 * (n + 4), 0xA5A5A5A5, np.uint32))
            ne = m.linearize_ct_device(desc, pb, pe, TB, TE, _params(prm), d_rows, d_xyz)
            got, moved = d_rows.download(np.uint8, 72 * (n + 4)), d_xyz.download(np.uint8, 12 * (n + 4))
            assert got[: 72 * n].tobytes() == want["rows"].tobytes(), tag
            assert moved[: 12 * n].tobytes() == want["moved"].tobytes(), tag
            assert np.all(got[72 * n :] == 0xA5) and np.all(moved[12 * n :] == 0xA5), tag
            assert (ne["n_used"], ne["n_found"], ne["n_outside"], ne["reserved"]) == (want["n_used"], want["n_found"], 0, 0), tag
            _check_sums(ne, ref, n, cauchy_a > 0, tag)
    _free(descs)
    d_rows.free(), d_xyz.free()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 513, N_SCAN])
def test_sizes(gpu, world, n):
    """the tile and wave edges, a second stage of more than 32 partials, and n = 0 (all zeros, status 0); from 63 points on with a NaN stamp,
    a stamp past t_end, and non-finite and out-of-range points in span"""
    m, surf = world["maps"][VS]
    body, times = world["body"][:n].copy(), world["times"][:n].copy()
    if n >= 63:
        times[5], times[40] = np.nan, TE + 1.0
        body[9], body[17], body[n - 1] = (np.nan, 0, 0), (0, np.inf, 0), (2.0**20 * VS * 1.5, 1, 1)
    prm = P(VS, cauchy_a=0.4)
    ne, rows, moved = m.linearize_ct(body, world["pb"], world["pe"], TB, TE, _params(prm), times=times, want_rows=True, want_xyz=True)
    if n == 0:
        assert not any(_bytes(ne)) and len(rows) == 0 and len(moved) == 0
        return
    want = CT.rows_ct(surf, body, times, world["pb"], world["pe"], TB, TE, VS, prm)
    assert rows.tobytes() == want["rows"].tobytes(), n
    fin = np.isfinite(body).all(1)
    assert moved[fin].tobytes() == want["moved"][fin].tobytes() and np.array_equal(np.isnan(moved), np.isnan(want["moved"])), n
    assert (ne["n_used"], ne["n_found"], ne["n_outside"]) == (want["n_used"], want["n_found"], want["n_outside"])
    if n >= 63:
        assert ne["n_outside"] == 2 and not rows[[5, 40, 9, 17, n - 1]].view(np.uint8).any() and want["n_used"] > 0
        assert np.isnan(moved[[5, 40]]).all()
    _check_sums(ne, CT.normal_eq_ct(want["rows"], want["w2"], 0.4), n, True, ("size", n))


def test_sums_are_formed_in_the_stated_order(gpu, world):
    """the order of every addition is wc_map_linearize's: the 75 weighted sums are, byte for byte, the float64 sums of the restated rows'
    terms formed in that order (map_register_ref.device_order_sum); without a loss rho = (w2 d) d has no log1p, and cost is held as well"""
    m, surf = world["maps"][0.2]
    for n, cauchy_a in ((257, 0.4), (N_SCAN, 0.4), (N_SCAN, 0.0)):
        prm = P(0.2, cauchy_a=cauchy_a)
        body, times = world["body"][:n], world["times"][:n]
        ne = m.linearize_ct(body, world["pb"], world["pe"], TB, TE, _params(prm), times=times)
        want = CT.linearize_ct(surf, body, times, world["pb"], world["pe"], TB, TE, 0.2, prm)
        for name, _ in CT.NAMES:
            assert ne[name].tobytes() == want[name].tobytes(), (n, name)
        assert (ne["n_used"], ne["n_found"], ne["n_outside"]) == (want["n_used"], want["n_found"], want["n_outside"])
        if cauchy_a == 0.0:
            assert ne["cost"] == want["cost"]


def test_determinism(gpu, world):
    """the 640 bytes: map_lin_groups 1, 3 and the default, both layouts, with and without d_rows and d_xyz_out - one value"""
    m, _ = world["maps"][0.2]
    n = N_SCAN
    prm = _params(P(0.2, cauchy_a=0.4))
    descs = _descs(gpu, world["body"], world["times"])
    d_rows, d_xyz = gpu.alloc(72 * n), gpu.alloc(12 * n)
    seen = set()
    try:
        for groups in (0, 1, 3, 0):
            gpu.set_dev_option("map_lin_groups", groups)
            for _, _, desc in descs:
                for rows, xyz in ((None, None), (d_rows, None), (None, d_xyz), (d_rows, d_xyz)):
                    seen.add(_bytes(m.linearize_ct_device(desc, world["pb"], world["pe"], TB, TE, prm, rows, xyz)))
    finally:
        gpu.set_dev_option("map_lin_groups", 0)
    assert len(seen) == 1
    ne = np.frombuffer(seen.pop(), R.MAP_CT_NORMAL_EQ)[0]
    assert ne["n_used"] > 1000 and ne["cost"] > 0
    _free(descs)
    d_rows.free(), d_xyz.free()


def test_stamp_edges(gpu, world):
    """every stamp = t_begin: a = 1 and s = 0 exactly, so H01, H11 and g1 are exactly zero and H00, g0 are the plain sums (k J_i) J_j,
    (k J_i) d in the stated order; every stamp = t_end: the mirror case.  One ulp outside either end and a NaN stamp: unused, counted
    in n_outside, a NaN triple in d_xyz_out; one ulp inside: used like any other"""
    m, surf = world["maps"][VS]
    n = 700
    body, pb, pe = world["body"][:n], world["pb"], world["pe"]
    prm = P(VS)
    for stamp, own, other in ((TB, ("H00", "g0"), ("H01", "H11", "g1")), (TE, ("H11", "g1"), ("H00", "H01", "g0"))):
        times = np.full(n, stamp)
        ne, rows = m.linearize_ct(body, pb, pe, TB, TE, _params(prm), times=times, want_rows=True)
        want = CT.rows_ct(surf, body, times, pb, pe, TB, TE, VS, prm)
        assert rows.tobytes() == want["rows"].tobytes() and ne["n_used"] == want["n_used"] > 300 and ne["n_outside"] == 0
        for name in other:
            assert not ne[name].view(np.uint8).any(), (stamp, name)  # (+0.0 in every entry)
        J, d, k = rows["J"], rows["d"], rows["k"]
        H = np.array([G.device_order_sum((k * J[:, a]) * J[:, b]) for a, b in G.UPPER])
        g = np.array([G.device_order_sum((k * J[:, a]) * d) for a in range(6)])
        assert ne[own[0]].tobytes() == H.tobytes() and ne[own[1]].tobytes() == g.tobytes(), stamp
    times = world["times"][:n].copy()
    out_idx, in_idx = [3, 100, 257, 600], [4, 101]
    times[out_idx] = [np.nextafter(TB, -np.inf), np.nextafter(TE, np.inf), np.nan, -np.inf]
    times[in_idx] = [np.nextafter(TB, np.inf), np.nextafter(TE, -np.inf)]
    ne, rows, moved = m.linearize_ct(body, pb, pe, TB, TE, _params(prm), times=times, want_rows=True, want_xyz=True)
    want = CT.rows_ct(surf, body, times, pb, pe, TB, TE, VS, prm)
    assert rows.tobytes() == want["rows"].tobytes() and moved.tobytes() == want["moved"].tobytes()
    assert ne["n_outside"] == 4 and not rows[out_idx].view(np.uint8).any()
    assert np.all(moved[out_idx].view(np.uint32) == 0x7FC00000) and np.isfinite(moved[in_idx]).all()
    assert np.array_equal(rows["s"][in_idx] > 0, want["used"][in_idx]) and want["used"][in_idx].any()


def test_moved_points_make_the_restatements_map(gpu, world):
    """d_xyz_out without its NaN rows, inserted into a fresh map, gives - through wc_map_export_state - bit for bit the map of the
    restatement's moved points; and wc_map_insert itself drops the NaN rows"""
    m, _ = world["maps"][VS]
    n = 3000
    body, times = world["body"][:n], world["times"][:n].copy()
    times[::7] = np.nan
    _, moved = m.linearize_ct(body, world["pb"], world["pe"], TB, TE, _params(P(VS)), times=times, want_xyz=True)
    want, _, inside = CT.interp_move(world["pb"], world["pe"], TB, TE, body, times)
    assert inside.sum() == n - len(times[::7])
    states = []
    for pts in (moved[~np.isnan(moved).any(1)], want[inside], moved):
        fresh = gpu.map_create(0.2, moments=True)
        assert fresh.insert(pts) == (0 if len(pts) < n else n - inside.sum())
        vox, mom = fresh.state()
        states.append((vox.tobytes(), mom.tobytes()))
        fresh.close()
    assert states[0] == states[1] == states[2] and len(states[0][0]) > 40 * 100


def _check_loop(got, want):
    """the library's loop against the restated one, digit for digit: every sum is formed in the stated order from rows that are equal
    byte for byte, the 12 x 12 solve and the pose update are the same IEEE operations (the C library's sine and cosine on both sides)"""
    (b1, e1, s1), (b2, e2, s2) = got, want
    print("loop: iterations", s1["iterations"], s2["iterations"], "termination", s1["termination"], "used", s1["n_used"], "cost", s1["initial_cost"],
          s1["final_cost"], "pose difference", max(np.abs(b1[0] - b2[0]).max(), np.abs(b1[1] - b2[1]).max(), np.abs(e1[0] - e2[0]).max(),
                                                 np.abs(e1[1] - e2[1]).max()))
    assert s1["iterations"] == s2["iterations"] and s1["termination"] == s2["termination"]
    for f in ("n_used", "n_found", "n_outside", "initial_cost", "final_cost", "prior_cost"):
        assert s1[f] == s2[f], f
    assert s1["last_step"].tobytes() == s2["last_step"].tobytes()
    for a, b in ((b1, b2), (e1, e2)):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_recovery_is_the_restatements_digit_for_digit(gpu, world):
    """the moving sweep of test_map_ct_ref (0.3 m and 6 degrees between the poses, v = 0.8f, no loss) from its perturbed starts: the
    iteration count, the summary and both poses of the restated loop on the map's own export; the truth is met as it is there, and the
    rigid registration of the same raw sweep ends further from the midpoint pose"""
    m, surf = world["maps"][VS]
    pb, pe = world["pb"], world["pe"]
    body, times = sweep_of(CT.N_SWEEP, pb, pe)
    pb0, pe0 = start_poses(pb, pe)
    kw = dict(max_iterations=30, tol_rot=CT.TOL_ROT, tol_trans=CT.TOL_TRANS)
    got = m.align_ct(body, pb0, pe0, TB, TE, params=_params(P(VS)), times=times, **kw)
    want = CT.align_ct(surf, body, times, pb0, pe0, TB, TE, VS, P(VS), **kw)
    _check_loop(got, want)
    b1, e1, summ = got
    assert summ["termination"] == 0 and summ["iterations"] >= 3 and summ["n_used"] > 0.95 * len(body)
    mid = CT.blend_pose(pb, pe, 0.5)
    errs = [CT.pose_error(b1, pb), CT.pose_error(CT.blend_pose(b1, e1, 0.5), mid), CT.pose_error(e1, pe)]
    T_rigid, s_rigid = m.align(body, CT.pose_T(CT.blend_pose(pb0, pe0, 0.5)), params=_params(P(VS)), **kw)
    e_rigid = G.pose_error(T_rigid, CT.pose_T(mid))
    print("recovery: continuous time", errs, "rigid", e_rigid, s_rigid["iterations"])
    for e_rot, e_tr in errs:
        assert e_rot < e_rigid[0] and e_tr < e_rigid[1]


def test_a_large_begin_prior_keeps_the_begin_pose(gpu, world):
    """prior (1e30, 1e30, 0, 0): the begin pose's steps are of the order g / 1e30 - the position is the input's bit for bit, the quaternion
    is renormalised by every update (at most one rounding per component and update) -, the end pose moves as before, and the loop is the
    restatement's digit for digit"""
    m, surf = world["maps"][VS]
    pb, pe = world["pb"], world["pe"]
    body, times = sweep_of(4000, pb, pe)
    pb0, pe0 = start_poses(pb, pe)
    kw = dict(max_iterations=6, tol_rot=CT.TOL_ROT, tol_trans=CT.TOL_TRANS, prior=(1e30, 1e30, 0.0, 0.0))
    got = m.align_ct(body, pb0, pe0, TB, TE, params=_params(P(VS)), times=times, **kw)
    _check_loop(got, CT.align_ct(surf, body, times, pb0, pe0, TB, TE, VS, P(VS), **kw))
    b1, e1, summ = got
    assert summ["iterations"] >= 2 and b1[0].tobytes() == pb0[0].tobytes()
    assert np.all(np.abs(b1[1] - pb0[1]) <= summ["iterations"] * 2.0**-52)
    assert np.abs(summ["last_step"][:6]).max() <= 1e-20 and CT.pose_error(e1, pe0)[1] > 1e-3 and summ["prior_cost"] <= 1e-6


def test_single_plane_map_ends_with_termination_2(gpu):
    """the hand wall: the scaled 12 x 12 matrix has zero diagonal entries -> termination 2, the poses untouched; with fewer used points than
    min_used likewise"""
    wall = G.hand_wall()
    m = gpu.map_create(G.HAND_V, moments=True)
    assert m.insert(wall) == 0
    scan = (wall.astype(np.float64) - np.array([0.0, 0.0, 1 / 64])).astype(np.float32)
    times = np.linspace(TB, TE, len(scan))
    I = (np.zeros(3), np.array([1.0, 0.0, 0.0, 0.0]))
    b1, e1, summ = m.align_ct(scan, I, I, TB, TE, params=_params(P(G.HAND_V, sigma0=2.0**-4)), times=times)
    assert summ["termination"] == 2 and summ["iterations"] == 0 and _bytes(b1[0]) + _bytes(b1[1]) == _bytes(I[0]) + _bytes(I[1])
    assert _bytes(e1[1]) == _bytes(I[1]) and summ["n_used"] == 36 and summ["initial_cost"] == summ["final_cost"] == 0.5 * 256 * 36 / 64**2
    assert not summ["last_step"].any()
    _, _, summ = m.align_ct(scan[:11], I, I, TB, TE, params=_params(P(G.HAND_V)), times=times[:11])
    assert summ["termination"] == 2 and summ["n_used"] == 11
    m.close()


def test_refused_arguments_leave_the_context_usable(gpu, world):
    m, _ = world["maps"][VS]
    lib = gpu.lib
    n = 2000
    body, times, pb, pe = world["body"][:n], world["times"][:n], world["pb"], world["pe"]
    d_xyz, d_t = gpu.to_device(body), gpu.to_device(times)
    desc = R.Points(d_xyz.ptr, d_t.ptr, 12, 8, n)
    good = _params(P(VS, cauchy_a=0.4))
    before = _bytes(m.linearize_ct_device(desc, pb, pe, TB, TE, good))
    out = np.full(80, 0x5A5A5A5A5A5A5A5A, np.uint64)
    sentinel = out.tobytes()

    def rc(ctx=gpu, mp=m, b=pb, e=pe, tb=TB, te=TE, prm=good, pts=desc, res=out, rows=0, xyz=0):
        bb, ee = (L._pose_rec(b) if b is not None else None), (L._pose_rec(e) if e is not None else None)
        return lib.wc_map_linearize_ct(ctx.h, mp.h if mp else None, C.byref(pts), C.byref(bb) if bb else None, C.byref(ee) if ee else None,
                                       C.c_double(tb), C.c_double(te), C.byref(prm) if prm else None, R.ptr(res) if res is not None else None,
                                       C.c_void_p(rows), C.c_void_p(xyz))

    def refused(**kw):
        assert rc(**kw) == WC_ERR_ARG, kw
        assert out.tobytes() == sentinel, kw

    assert rc() == 0 and out.tobytes() == before
    out[:] = 0x5A5A5A5A5A5A5A5A
    refused(pts=R.Points(d_xyz.ptr, 0, 12, 8, n))  # no stamps
    # optional outputs that are not aligned: d_rows to 8 bytes, d_xyz_out to 4 (the buffers stay as they are)
    d_opt = gpu.alloc(72 * n + 16)
    d_opt.upload(np.full(18 * n + 4, 0xA5A5A5A5, np.uint32))
    refused(rows=d_opt.ptr + 4), refused(rows=d_opt.ptr + 1), refused(xyz=d_opt.ptr + 2), refused(xyz=d_opt.ptr + 1)
    assert np.all(d_opt.download(np.uint8, 72 * n + 16) == 0xA5)
    assert rc(rows=d_opt.ptr + 8, xyz=0) == 0 and out.tobytes() == before  # (8-aligned is enough)
    out[:] = 0x5A5A5A5A5A5A5A5A
    d_opt.free()
    refused(pts=R.Points(d_xyz.ptr, d_t.ptr, 12, 0, n)), refused(pts=R.Points(d_xyz.ptr, d_t.ptr, 12, 12, n)), refused(pts=R.Points(d_xyz.ptr, d_t.ptr + 4, 12, 8, n))
    for bad in (np.nan, np.inf, -np.inf):
        for j in range(7):
            p = np.concatenate([pb[0], pb[1]])
            p[j] = bad
            refused(b=p), refused(e=p)
    refused(b=(pb[0], np.zeros(4))), refused(e=(pe[0], np.zeros(4))), refused(b=None), refused(e=None)
    refused(te=TB), refused(te=TB - 0.1), refused(tb=np.nan), refused(te=np.nan), refused(tb=-np.inf), refused(te=np.inf)
    plain = gpu.map_create(VS)
    plain.insert(body)
    refused(mp=plain)  # a map without moments
    plain.close()
    other = L.Context(0)
    refused(ctx=other)  # a map of another context
    other.close()
    refused(mp=None), refused(prm=None)
    assert rc(res=None) == WC_ERR_ARG
    check_unreadable_points_refused(gpu, lambda bad: rc(pts=R.Points(bad.xyz, d_t.ptr, bad.xyz_stride, 8, bad.n)))
    for kw in (dict(max_dist=0.0), dict(max_dist=np.nan), dict(min_points=2), dict(sigma0=0.0), dict(sigma0=np.inf), dict(cauchy_a=-0.4),
               dict(cauchy_a=np.nan)):
        base = dict(max_dist=VS, min_points=3, sigma0=0.05 / 6, cauchy_a=0.4)
        base.update(kw)
        refused(prm=L.map_reg_params(**base))
    reserved = L.map_reg_params(VS)
    reserved.reserved = 1
    refused(prm=reserved)
    # poses that send finite points to non-finite ones: a position beyond float (1e39 m; the largest float is 3.4e38) and near double's end
    for big in (1e39, 1e308):
        assert rc(b=(pb[0] * 0 + big, pb[1])) == WC_ERR_ARG, big
        assert _bytes(m.linearize_ct_device(desc, pb, pe, TB, TE, good)) == before
    # the loop's options
    summ = R.MapCtAlignSummary()
    for kw in (dict(max_iterations=0), dict(tol_rot=0.0), dict(tol_trans=np.nan), dict(min_used=11), dict(min_pivot=0.0), dict(prior=(0, -1.0, 0, 0)),
               dict(prior=(0, 0, np.inf, 0)), dict(prior=(np.nan, 0, 0, 0))):
        opts = L.map_ct_align_opts(good, **kw)
        bb, ee = L._pose_rec(pb), L._pose_rec(pe)
        assert lib.wc_map_align_ct(gpu.h, m.h, C.byref(desc), C.byref(bb), C.byref(ee), C.c_double(TB), C.c_double(TE), C.byref(opts),
                                   C.byref(summ)) == WC_ERR_ARG, kw
        assert list(bb.quat) == list(pb[1]) and list(ee.pos) == list(pe[0])
    # ... and the context still computes what it computed before
    assert _bytes(m.linearize_ct_device(desc, pb, pe, TB, TE, good)) == before
    d_xyz.free(), d_t.free()


def test_facade(gpu):
    """Odometry.map_align_sweep on a short room stream equals the direct calls on a stand-alone moments map fed the same published
    sweeps; with insert the map gains exactly the registered points; a miss with map_surfels off"""
    msgs, imu, _ = synth.raw_stream(1.7, pts_per_s=300_000, gyro_bias=(0.0, 0.0, 0.02), t_start=1000.0)
    v = 0.1
    odo = L.Odometry(0)
    odo.set_fill_outputs(True)
    odo.set_map_voxel(v)
    odo.set_map_surfels(True)
    scans = []
    _drive(odo, msgs, imu, lambda: scans.append(_xyz(odo.outputs()["scan"])))
    assert odo.sweeps() >= 2
    ref = gpu.map_create(v, moments=True)
    for s in scans:
        assert ref.insert(s) == 0
    # the last published sweep, thinned, measured again from a sensor that moves 5 cm and 1 degree
    pb = (np.array([0.01, -0.02, 0.005]), CT.quat_of_rotvec(np.array([0.0, 0.0, np.deg2rad(0.3)])))
    pe = CT.pose_update_ct(pb, np.array([0.002, -0.004, np.deg2rad(1.0), 0.04, 0.03, 0.0]))
    body, times = CT.simulate_sweep(scans[-1][::3], pb, pe, 2000.0, 2000.1)
    pts = synth.make_points(body, times)
    pb0, pe0 = CT.pose_update_ct(pb, np.array([0.001, 0.0, -0.002, 0.01, -0.01, 0.005])), CT.pose_update_ct(pe, np.array([0.0, 0.002, 0.001, -0.01, 0.0, 0.01]))
    opts = L.map_ct_align_opts(L.map_reg_params(2 * v, 3, cauchy_a=0.4), max_iterations=4)
    got = odo.map_align_sweep(pts, pb0, pe0, opts)
    want = ref.align_ct(pts, pb0, pe0, times.min(), times.max(), opts)
    assert got is not None and got[2]["iterations"] >= 1 and got[2]["n_used"] > 100
    for a, b in ((got[0], want[0]), (got[1], want[1])):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    for f in ("initial_cost", "final_cost", "iterations", "termination", "n_used", "n_found", "n_outside", "prior_cost"):
        assert got[2][f] == want[2][f], f
    assert got[2]["last_step"].tobytes() == want[2]["last_step"].tobytes()
    # insert: the map gains exactly the moved points of the linearisation at the final poses
    before = odo.map_size()
    got2 = odo.map_align_sweep(pts, pb0, pe0, opts, insert=True)
    assert got2[0][1].tobytes() == got[0][1].tobytes() and got2[1][0].tobytes() == got[1][0].tobytes()
    _, moved = ref.linearize_ct(pts, got[0], got[1], times.min(), times.max(), opts.reg, want_xyz=True)
    assert not np.isnan(moved).any() and ref.insert(moved) == 0
    assert odo.map_size()[1] == before[1] + len(pts)
    xyz_o, cnt_o = odo.map_export()
    xyz_r, cnt_r, _ = ref.export()
    assert xyz_o.tobytes() == xyz_r.tobytes() and cnt_o.tobytes() == cnt_r.tobytes()
    # misses, not aborts: refused options, an empty sweep, a sweep without a stamp interval, no moments, no map
    assert odo.map_align_sweep(pts, pb0, pe0, L.map_ct_align_opts(L.map_reg_params(2 * v, 2))) is None
    assert odo.map_align_sweep(pts[:0], pb0, pe0, opts) is None
    assert odo.map_align_sweep(synth.make_points(body, np.full(len(body), 7.0)), pb0, pe0, opts) is None
    ref.close()
    odo.set_map_surfels(False)
    assert odo.map_align_sweep(pts, pb0, pe0, opts) is None
    odo.set_map_voxel(0.0)
    assert odo.map_align_sweep(pts, pb0, pe0, opts) is None
    odo.close()
