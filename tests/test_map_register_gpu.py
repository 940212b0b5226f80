"""Registration against the voxel map on the device (wc_map_linearize, wc_map_align, csrc/map.hip: k_map_linearize<true>, k_map_lin_reduce)
against the restatement of map_register_ref.py on the map's own export: the rows byte for byte, the sums within the bound their
additions allow, determinism over runs, grids, layouts and outputs, one Gauss-Newton step by its backward error, the recovery of a known
pose, the refused arguments and the facade."""
import ctypes as C

import numpy as np
import pytest

import map_register_ref as G
from extract_ref import LD
from helpers import check_unreadable_points_refused, point_records as _records, xyz_of as _xyz
from test_map_gpu import _drive
from test_map_register_ref import P, scan_of, true_pose
from wildcat_slam_amd import lib as L
from wildcat_slam_amd import records as R
from wildcat_slam_amd import synth

pytestmark = pytest.mark.gpu

EPS = G.EPS
VS = float(np.float32(0.8))
WC_ERR_ARG = 11
N_SCAN = 256 * 33 + 7  # 34 tiles: a second stage with more than 32 partials, a ragged last tile
# the error of fp64 log1p: HIP documentation, "HIP math API", table "Double precision mathematical functions": log1p, maximum error
# 1 ULP - at most 2 x 2^-53 of the value
LOG1P_EPS = 2
# roundings of one term of cost besides its additions: (w2 d) d (2), s / a^2 (1), a^2 * (1), the condition number of log1p is <= 1
COST_ROUNDINGS = 4


def _params(p):
    return L.map_reg_params(p.max_dist, p.min_points, p.sigma0, p.cauchy_a)


def _ne_bytes(ne):
    return np.asarray(ne).tobytes()


@pytest.fixture(scope="module")
def world(gpu):
    """the maps (g1_room at v = 0.2 and 0.8f, the hand corner), their exports, the scan and the true pose"""
    room = _xyz(synth.g1_room(200_000))
    maps = {}
    for v in (0.2, VS):
        m = gpu.map_create(v, moments=True)
        assert m.insert(room) == 0
        maps[v] = (m, m.surfels())
    T = true_pose()
    yield dict(maps=maps, T=T, scan=scan_of(N_SCAN, T))
    for m, _ in maps.values():
        m.close()


def _descs(gpu, scan):
    """both point layouts of a scan -> [(name, buffer, wc_points)]"""
    d12, d48 = gpu.to_device(scan), gpu.to_device(_records(scan))
    return [("xyz12", d12, R.Points(d12.ptr, 0, 12, 0, len(scan))), ("point48", d48, R.Points(d48.ptr, d48.ptr + 24, 48, 48, len(scan)))]


def _check_sums(ne, ref, n, loss, what):
    """|gpu - ref| <= (A(n) + 3) 2^-53 sum |term| on every entry of H and g: a term (k J_a) J_b carries two roundings, its way into the
    sum at most A(n) additions, each (1 + delta), |delta| <= 2^-53: to first order (A(n) + 2) 2^-53 |term|, and one more 2^-53 covers
    the second-order terms ((A + 2)^2 2^-106 < 2^-53 for A <= 128) and the reference's own longdouble roundings.  cost: a term carries
    COST_ROUNDINGS roundings and, with the loss, log1p's documented error instead of two"""
    A = G.adds_bound(n)
    print(what, "A(n) =", A)
    for name, got, want, scale in (("H", ne["H"], ref["H"], ref["absH"]), ("g", ne["g"], ref["g"], ref["absg"])):
        err = np.abs(got.astype(LD) - want)
        bound = (A + 3) * EPS * scale
        print("  ", name, "max |gpu - ref| / bound =", float(np.max(err / np.where(bound > 0, bound, 1))))
        assert np.all(err <= bound), (what, name, err, bound)
    roundings = COST_ROUNDINGS + LOG1P_EPS if loss else 2
    err, bound = abs(LD(ne["cost"]) - ref["cost"]), (A + roundings + 1) * EPS * ref["abscost"]
    print("   cost |gpu - ref| / bound =", float(err / bound) if bound > 0 else 0.0)
    assert err <= bound, (what, "cost", err, bound)


@pytest.mark.parametrize("v", [0.2, VS])
def test_rows_are_the_restatement_byte_for_byte(gpu, world, v):
    """identity and the true pose, the Cauchy loss off and on, min_points 3 and 10, both point layouts: d_rows equals rows() byte for
    byte, n_used and n_found equal the restatement's, n_found equals nearest_plane's on the moved points, the bytes behind the n rows
    are untouched; and the sums of every configuration meet their bound"""
    m, surf = world["maps"][v]
    scan, n = world["scan"], N_SCAN
    descs = _descs(gpu, scan)
    d_rows = gpu.alloc(64 * (n + 4))
    used_counts = []
    for T in (np.eye(3, 4), world["T"]):
        q = G.transform(scan, T)
        d_q = gpu.to_device(q)
        d_hits = gpu.alloc(80 * n)
        n_near = m.nearest_plane_device(R.Points(d_q.ptr, 0, 12, 0, n), v, 3, d_hits)
        for b in (d_q, d_hits):
            b.free()
        for cauchy_a in (0.0, 0.4):
            for min_points in (3, 10):
                prm = P(v, min_points=min_points, cauchy_a=cauchy_a)
                want = G.rows_ex(surf, scan, T, v, prm)
                ref = G.normal_eq(want["rows"], want["w2"], cauchy_a)
                used_counts.append(want["n_used"])
                for name, _, desc in descs:
                    tag = (v, T[0, 0], cauchy_a, min_points, name)
                    d_rows.upload(np.full(16 * (n + 4), 0xA5A5A5A5, np.uint32))
                    ne = m.linearize_device(desc, T, _params(prm), d_rows)
                    got = d_rows.download(np.uint8, 64 * (n + 4))
                    assert got[: 64 * n].tobytes() == want["rows"].tobytes(), tag
                    assert np.all(got[64 * n :] == 0xA5), tag
                    assert ne["n_used"] == want["n_used"] and ne["n_found"] == want["n_found"] == n_near, tag
                    _check_sums(ne, ref, n, cauchy_a > 0, tag)
    assert min(used_counts) > 1000 and len(set(used_counts)) > 2, used_counts
    for _, b, _ in descs:
        b.free()
    d_rows.free()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 513, N_SCAN])
def test_sizes(gpu, world, n):
    """the tile and wave edges, a second stage of more than 32 partials, and n = 0 (all zeros, status 0); every size with some points
    replaced by NaN, infinite and out-of-range ones"""
    m, surf = world["maps"][VS]
    scan = world["scan"][:n].copy()
    if n >= 63:
        scan[5], scan[17], scan[n - 1] = (np.nan, 0, 0), (0, np.inf, 0), (2.0**20 * VS * 1.5, 1, 1)
    prm = P(VS, cauchy_a=0.4)
    ne, rows = m.linearize(scan, world["T"], _params(prm), want_rows=True)
    if n == 0:
        assert not any(_ne_bytes(ne)) and len(rows) == 0
        return
    want = G.rows_ex(surf, scan, world["T"], VS, prm)
    assert rows.tobytes() == want["rows"].tobytes(), n
    assert ne["n_used"] == want["n_used"] and ne["n_found"] == want["n_found"]
    if n >= 63:
        assert not rows[[5, 17, n - 1]].view(np.uint8).any() and want["n_used"] > 0
    _check_sums(ne, G.normal_eq(want["rows"], want["w2"], 0.4), n, True, ("size", n))


def test_a_scan_without_planes(gpu, world):
    """a scan a kilometre away: nothing found, nothing used, H, g and cost exactly zero; the hand corner's map with min_points above
    every count: found but not used"""
    m, _ = world["maps"][VS]
    far = world["scan"][:1000] + np.float32(1000.0)
    ne, rows = m.linearize(far, np.eye(3, 4), _params(P(VS)), want_rows=True)
    assert not any(_ne_bytes(ne)) and not rows.view(np.uint8).any()
    pts, _ = G.hand_corner()
    hand = gpu.map_create(G.HAND_V, moments=True)
    assert hand.insert(pts) == 0
    ne = hand.linearize(pts, np.eye(3, 4), _params(P(G.HAND_V, min_points=10)))
    assert ne["n_found"] == len(pts) and ne["n_used"] == 0 and not ne["H"].any() and not ne["g"].any() and ne["cost"] == 0
    hand.close()


def test_hand_corner(gpu):
    """the hand map of test_map_register_ref.py on the device: exact planes, exact sums (every term is dyadic), one step recovers the
    translation, the loop converges in two steps"""
    pts, axis = G.hand_corner()
    hand = gpu.map_create(G.HAND_V, moments=True)
    assert hand.insert(pts) == 0
    surf = hand.surfels()
    assert len(surf) == 12 and np.all(surf["count"] == 9) and np.all(surf["flags"] == 1) and not surf["ev"][:, 0].any()
    assert sorted(map(tuple, surf["normal"].tolist())) == sorted([(1.0, 0.0, 0.0)] * 4 + [(0.0, 1.0, 0.0)] * 4 + [(0.0, 0.0, 1.0)] * 4)
    delta = np.array([1 / 64, -1 / 32, 1 / 128])
    scan = (pts.astype(np.float64) - delta).astype(np.float32)
    prm = P(G.HAND_V, sigma0=2.0**-4)
    ne, rows = hand.linearize(scan, np.eye(3, 4), _params(prm), want_rows=True)
    assert rows.tobytes() == G.rows(surf, scan, np.eye(3, 4), G.HAND_V, prm).tobytes()
    H, g, cost, n_used, n_found = G.linearize(surf, scan, np.eye(3, 4), G.HAND_V, prm)
    assert ne["H"].tobytes() == H.tobytes() and ne["g"].tobytes() == g.tobytes() and ne["cost"] == cost and ne["n_used"] == n_used == 108
    assert np.array_equal(G.full(ne["H"])[3:, 3:], 256.0 * 36 * np.eye(3))
    T1, summ = hand.align(scan, np.eye(3, 4), params=_params(prm), max_iterations=5, tol_rot=1e-9, tol_trans=1e-9)
    assert summ["termination"] == 0 and summ["iterations"] == 2 and summ["final_cost"] <= 1e-20 and summ["n_used"] == 108
    assert np.all(np.abs(T1 - np.concatenate([np.eye(3), delta[:, None]], 1)) <= 1e-12)
    hand.close()


def test_sums_are_formed_in_the_stated_order(gpu, world):
    """more than the bound: the header fixes the order of every addition, so H and g are, byte for byte, the float64 sums of the
    restated rows' terms formed in that order (map_register_ref.device_order_sum); cost is not held this way, log1p is not bit exact"""
    m, surf = world["maps"][0.2]
    prm = P(0.2, cauchy_a=0.4)
    for n in (257, N_SCAN):
        scan = world["scan"][:n]
        ne = m.linearize(scan, world["T"], _params(prm))
        H, g, _, n_used, n_found = G.linearize(surf, scan, world["T"], 0.2, prm)
        assert ne["H"].tobytes() == H.tobytes() and ne["g"].tobytes() == g.tobytes(), n
        assert (ne["n_used"], ne["n_found"]) == (n_used, n_found)


def test_determinism(gpu, world):
    """the 240 bytes: two runs, map_lin_groups 1, 7 and the default, with and without d_rows, both layouts - one value"""
    m, _ = world["maps"][0.2]
    scan, n = world["scan"], N_SCAN
    prm = _params(P(0.2, cauchy_a=0.4))
    descs = _descs(gpu, scan)
    d_rows = gpu.alloc(64 * n)
    seen = set()
    try:
        for groups in (0, 1, 7, 0):
            gpu.set_dev_option("map_lin_groups", groups)
            for _, _, desc in descs:
                for rows in (None, d_rows):
                    seen.add(_ne_bytes(m.linearize_device(desc, world["T"], prm, rows)))
    finally:
        gpu.set_dev_option("map_lin_groups", 0)
    assert len(seen) == 1
    ne = np.frombuffer(seen.pop(), R.MAP_NORMAL_EQ)[0]
    assert ne["n_used"] > 1000 and ne["cost"] > 0
    for _, b, _ in descs:
        b.free()
    d_rows.free()


def test_one_step(gpu, world):
    """max_iterations = 1 from identity: last_step against the longdouble sums H, g of the restated rows, by the residual of the
    unit-diagonal system  A y = b,  A = D H D,  b = -D g,  D = diag(H)^-1/2,  y = D^-1 xi  (all formed in longdouble from the reference).
    What the library solves is a perturbed system, (A~ + dA) y^ = b~, xi^ = fl(D~ y^):
      sums       |H~_ab - H_ab| <= beta absH_ab, |g~_a - g_a| <= beta absg_a, beta = (A(n) + 3) 2^-53 (test_rows' bound); the weights k
                 are positive, so absH_aa = H_aa and, by Cauchy-Schwarz, absH_ab <= sqrt(H_aa H_bb), absg_a <= sqrt(H_aa) S, S^2 = sum k d^2
      scaling    D~_a = fl(1 / fl(sqrt(H~_aa))): relative error beta / 2 + 2u (u = 2^-53); A~_ab = fl(fl(D~_a H~_ab) D~_b), the diagonal
                 exactly 1: |A~_ab - A_ab| <= beta + (beta + 6u) = 2 beta + 6u off the diagonal, 30 entries:
                 |A~ - A|_2 <= sqrt(30) (2 beta + 6u);   b~_a = fl(D~_a g~_a): |b~ - b|_2 <= sqrt(6) (3 beta / 2 + 3u) S
      Cholesky   Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Theorem 10.4: |dA| <= gamma_(3n+1) |R^T| |R|, and
                 (10.7) | |R^T| |R| |_2 <= n (1 - n gamma_(n+1))^-1 |A~|_2: with n = 6, |dA|_2 <= 6 gamma_19 / (1 - 6 gamma_7) |A~|_2
      unscaling  y = D^-1 xi^ = y^ (1 + e), |e| <= beta / 2 + 3u
    so  |A y - b|_2 <= [ sqrt(30) (2 beta + 6u) + (6 gamma_19 / (1 - 6 gamma_7) + beta / 2 + 3u) |A|_2 ] |y|_2 + sqrt(6) (3 beta / 2 + 3u) S,
    times 1.01 for the second-order terms (products of quantities below 1e-13).  Nothing here is measured.
    T_io is the restated update of last_step, to 8 x 2^-53 of the largest entry of T (a 3 x 3 product of entries formed with sin)."""
    m, surf = world["maps"][VS]
    scan, n = world["scan"], N_SCAN
    prm = P(VS, cauchy_a=0.4)
    T0 = np.eye(3, 4)
    T1, summ = m.align(scan, T0, params=_params(prm), max_iterations=1, tol_rot=1e-12, tol_trans=1e-12)
    assert summ["iterations"] == 1 and summ["termination"] == 1
    r = G.rows_ex(surf, scan, T0, VS, prm)
    ref = G.normal_eq(r["rows"], r["w2"], 0.4)
    assert summ["n_used"] > 1000 and abs(summ["initial_cost"] - float(ref["cost"])) <= 1e-12 * float(ref["cost"])
    H, g = G.full(ref["H"]), ref["g"]
    D = 1 / np.sqrt(np.diag(H))
    A, b = H * D[:, None] * D[None, :], -(D * g)
    y = summ["last_step"].astype(LD) / D
    u = LD(EPS)
    beta = (G.adds_bound(n) + 3) * u
    S = np.sqrt(G.comp_sum(r["rows"]["k"].astype(LD) * r["rows"]["d"].astype(LD) ** 2))
    gam = lambda k: k * u / (1 - k * u)  # noqa: E731
    normA = LD(np.linalg.norm(A.astype(np.float64), 2)) * (1 + 1e-12)
    norm2 = lambda x: np.sqrt((x * x).sum())  # noqa: E731
    bound = ((np.sqrt(LD(30)) * (2 * beta + 6 * u) + (6 * gam(19) / (1 - 6 * gam(7)) + beta / 2 + 3 * u) * normA) * norm2(y)
             + np.sqrt(LD(6)) * (1.5 * beta + 3 * u) * S) * LD(1.01)
    res = norm2(A @ y - b)
    print("one step: |A y - b| / bound =", float(res / bound), "|xi| =", float(norm2(summ["last_step"])), "|A|_2 =", float(normA))
    assert res <= bound
    want = G.pose_update(T0, summ["last_step"])
    assert np.all(np.abs(T1 - want) <= 8 * EPS * np.abs(want).max()), np.abs(T1 - want).max()
    assert np.linalg.norm(summ["last_step"][3:]) > 0.01  # (a real step: the scan starts 6 cm and 2 degrees off)


def test_recovery(gpu, world):
    """the full loop from identity at v = 0.8f without a loss (with the Cauchy loss the loop is an iteratively reweighted one and
    converges linearly: no tolerance is met 10 x under), against the float64 restatement on the same export: termination 0, the pose
    error at most twice the restatement's in angle and in translation (a correspondence may differ on an exact tie; the error itself is
    set by the 2^-16 m grid, the voxel size and the sampling noise, not by arithmetic), the iteration count within one"""
    m, surf = world["maps"][VS]
    T = world["T"]
    scan = scan_of(G.N_ALIGN, T)
    kw = dict(max_iterations=30, tol_rot=G.TOL_ROT, tol_trans=G.TOL_TRANS)
    T_gpu, s_gpu = m.align(scan, np.eye(3, 4), params=_params(P(VS)), **kw)
    T_ref, s_ref = G.align(surf, scan, np.eye(3, 4), VS, P(VS), **kw)
    e_gpu, e_ref = G.pose_error(T_gpu, T), G.pose_error(T_ref, T)
    print("recovery: gpu", e_gpu, s_gpu["iterations"], "restatement", e_ref, s_ref["iterations"], "last steps", s_gpu["last_step"], s_ref["last_step"])
    assert s_gpu["termination"] == 0 and s_ref["termination"] == 0
    assert np.linalg.norm(s_ref["last_step"][:3]) <= G.TOL_ROT / 10 and np.linalg.norm(s_ref["last_step"][3:]) <= G.TOL_TRANS / 10
    assert e_gpu[0] <= 2 * e_ref[0] and e_gpu[1] <= 2 * e_ref[1]
    assert abs(s_gpu["iterations"] - s_ref["iterations"]) <= 1
    assert e_ref[0] < np.deg2rad(0.1) and e_ref[1] < 0.01 and s_gpu["final_cost"] < s_gpu["initial_cost"]
    assert s_gpu["n_used"] > 0.9 * len(scan) and s_gpu["n_found"] >= s_gpu["n_used"]


def test_refused_arguments_leave_the_context_usable(gpu, world):
    m, _ = world["maps"][VS]
    lib = gpu.lib
    scan = world["scan"][:2000]
    d = gpu.to_device(scan)
    desc = R.Points(d.ptr, 0, 12, 0, len(scan))
    good = _params(P(VS, cauchy_a=0.4))
    I = np.eye(3, 4)
    before = _ne_bytes(m.linearize_device(desc, I, good))
    out = np.zeros(1, R.MAP_NORMAL_EQ)

    def rc(ctx=gpu, mp=m, T=I, prm=good, pts=desc):
        T = np.ascontiguousarray(np.asarray(T, np.float64).reshape(-1))
        return lib.wc_map_linearize(ctx.h, mp.h if mp else None, C.byref(pts), R.ptr(T), C.byref(prm) if prm else None, R.ptr(out), None)

    assert rc() == 0
    for j in (0, 5, 11):  # a non-finite entry of T
        for bad in (np.nan, np.inf, -np.inf):
            T = I.copy().reshape(-1)
            T[j] = bad
            assert rc(T=T) == WC_ERR_ARG, (j, bad)
    # a T that sends finite points to non-finite ones: beyond double (1e308 x 10 m) and beyond float (1e38 x 10 m)
    for big in (1e308, 1e38):
        assert rc(T=I * big) == WC_ERR_ARG, big
        assert _ne_bytes(m.linearize_device(desc, I, good)) == before
    plain = gpu.map_create(VS)
    plain.insert(scan)
    assert rc(mp=plain) == WC_ERR_ARG  # a map without moments
    with pytest.raises(L.WildcatError):
        plain.linearize(scan, I)
    with pytest.raises(L.WildcatError):
        plain.align(scan, I)
    plain.close()
    other = L.Context(0)
    assert rc(ctx=other) == WC_ERR_ARG  # a map of another context
    other.close()
    assert rc(mp=None) == WC_ERR_ARG and rc(prm=None) == WC_ERR_ARG
    check_unreadable_points_refused(gpu, lambda bad: rc(pts=bad))
    for kw in (dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=np.nan), dict(min_points=2), dict(sigma0=0.0), dict(sigma0=np.nan),
               dict(sigma0=np.inf), dict(sigma0=-1.0), dict(cauchy_a=-0.4), dict(cauchy_a=np.nan), dict(cauchy_a=np.inf)):
        base = dict(max_dist=VS, min_points=3, sigma0=0.05 / 6, cauchy_a=0.4)
        base.update(kw)
        assert rc(prm=L.map_reg_params(**base)) == WC_ERR_ARG, kw
    reserved = L.map_reg_params(VS)
    reserved.reserved = 1
    assert rc(prm=reserved) == WC_ERR_ARG
    assert rc(prm=L.map_reg_params(np.inf)) == 0  # (max_dist = +inf is allowed)
    # the loop's options
    summ, T = R.MapAlignSummary(), np.ascontiguousarray(I.reshape(-1))
    for kw in (dict(max_iterations=0), dict(tol_rot=0.0), dict(tol_trans=np.nan), dict(min_used=5), dict(min_pivot=0.0), dict(min_pivot=-1.0)):
        opts = L.map_align_opts(good, **kw)
        assert lib.wc_map_align(gpu.h, m.h, C.byref(desc), R.ptr(T), C.byref(opts), C.byref(summ)) == WC_ERR_ARG, kw
    bad_T = T.copy()
    bad_T[3] = np.nan
    assert lib.wc_map_align(gpu.h, m.h, C.byref(desc), R.ptr(bad_T), C.byref(L.map_align_opts(good)), C.byref(summ)) == WC_ERR_ARG
    assert np.array_equal(T, I.reshape(-1))
    # ... and the context still computes what it computed before
    assert _ne_bytes(m.linearize_device(desc, I, good)) == before
    d.free()


def test_single_plane_map_ends_with_termination_2(gpu):
    """the hand wall: three pose directions are free, the scaled matrix has non-finite entries -> termination 2, T_io unchanged"""
    wall = G.hand_wall()
    m = gpu.map_create(G.HAND_V, moments=True)
    assert m.insert(wall) == 0
    scan = (wall.astype(np.float64) - np.array([0.0, 0.0, 1 / 64])).astype(np.float32)
    T0 = np.eye(3, 4)
    T1, summ = m.align(scan, T0, params=_params(P(G.HAND_V, sigma0=2.0**-4)))
    assert summ["termination"] == 2 and summ["iterations"] == 0 and T1.tobytes() == T0.tobytes()
    assert summ["n_used"] == 36 and summ["initial_cost"] == summ["final_cost"] == 0.5 * 256 * 36 / 64**2 and not summ["last_step"].any()
    _, summ = m.align(scan[:5], T0, params=_params(P(G.HAND_V)))  # fewer used points than min_used
    assert summ["termination"] == 2 and summ["n_used"] == 5
    m.close()


def test_facade(gpu):
    """Odometry.map_linearize / map_align on a short room stream equal a stand-alone moments map fed the same published sweeps, byte
    for byte; both miss with map_surfels off"""
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
    q = scans[-1][::3]
    w = np.deg2rad(0.3) * np.array([0.0, 0.0, 1.0])
    T = np.concatenate([G.rodrigues(w), np.array([[0.01], [-0.02], [0.005]])], 1)
    prm = L.map_reg_params(2 * v, 3, cauchy_a=0.4)
    ne, rows = odo.map_linearize(q, T, prm, want_rows=True)
    ne_ref, rows_ref = ref.linearize(q, T, prm, want_rows=True)
    assert _ne_bytes(ne) == _ne_bytes(ne_ref) and rows.tobytes() == rows_ref.tobytes() and ne["n_used"] > 100
    assert _ne_bytes(odo.map_linearize(q, T, prm)) == _ne_bytes(ne_ref)
    opts = L.map_align_opts(prm, max_iterations=4)
    T_odo, s_odo = odo.map_align(q, T, opts)
    T_ref, s_ref = ref.align(q, T, opts)
    assert T_odo.tobytes() == T_ref.tobytes() and s_odo["iterations"] == s_ref["iterations"] >= 1
    for f in ("initial_cost", "final_cost", "termination", "n_used", "n_found"):
        assert s_odo[f] == s_ref[f], f
    assert s_odo["last_step"].tobytes() == s_ref["last_step"].tobytes()
    # refused arguments are a miss, not an abort
    assert odo.map_linearize(q, T, L.map_reg_params(2 * v, 2)) is None
    ref.close()
    odo.set_map_surfels(False)
    assert odo.map_linearize(q, T, prm) is None and odo.map_align(q, T, opts) is None
    odo.set_map_voxel(0.0)
    assert odo.map_linearize(q, T, prm) is None and odo.map_align(q, T, opts) is None
    odo.close()
