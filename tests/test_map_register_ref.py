"""Registration against the voxel map (include/wildcat_hip.h: wc_map_linearize, wc_map_align) - the parts that need no GPU: the
restatement of map_register_ref.py against finite differences, a hand-worked corner, a degenerate map, the declared interface, and the
proof that the GPU test's bound on the sums is tight enough to catch single-precision sums and a dropped tile."""
import ctypes as C
import os
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

import map_register_ref as G
from extract_ref import LD
from helpers import xyz_of as _xyz
from test_map_surfel_ref import _c_fields
from wildcat_slam_amd import records as R
from wildcat_slam_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = G.EPS
VS = float(np.float32(0.8))


def P(max_dist, min_points=3, sigma0=0.05 / 6, cauchy_a=0.0):
    return SimpleNamespace(max_dist=max_dist, min_points=min_points, sigma0=sigma0, cauchy_a=cauchy_a)


def true_pose():
    """the issue's pose: 2 degrees about (1, 2, 3) / |.|, translation (0.05, -0.03, 0.02) m -> (3, 4)"""
    axis = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    return np.concatenate([G.rodrigues(np.deg2rad(2.0) * axis), np.array([[0.05], [-0.03], [0.02]])], 1)


def scan_of(n, T):
    """g1_room(n, seed + 7) moved by the inverse of T, as float32: T maps the scan back onto the room"""
    p = _xyz(synth.g1_room(n, seed=synth.SEED + 7)).astype(np.float64)
    return ((p - T[:, 3]) @ T[:, :3]).astype(np.float32)  # R^T (p - t)


@pytest.fixture(scope="module")
def room():
    return G.surfels_cpu(_xyz(synth.g1_room(200_000)), VS)


def test_adds_bound():
    """A(n) of the header, and its condition A(n) <= 128 for n <= 2^20"""
    assert [G.adds_bound(n) for n in (0, 1, 256, 257, 8192, 8193, 2**18, 2**20)] == [0, 38, 38, 39, 69, 70, 100, 103]
    assert max(G.adds_bound(n) for n in list(range(1, 70000, 97)) + [2**20 - k * 255 for k in range(4000)]) <= 128


def test_device_order_sum_stays_within_its_additions():
    """the restated device order against the compensated sum: |error| <= (A(n) + 1) 2^-53 sum |x|"""
    for n in (1, 255, 257, 256 * 33 + 7):
        x = np.random.Generator(np.random.PCG64(n)).normal(size=n)
        assert abs(LD(G.device_order_sum(x)) - G.comp_sum(x)) <= (G.adds_bound(n) + 1) * EPS * np.abs(x).sum(), n


@pytest.mark.parametrize("cauchy_a", [0.0, 0.4])
def test_jacobian_against_central_differences(room, cauchy_a):
    """On FIXED planes - the normal n and centroid c each used point was matched to - the residual of a perturbed pose is
        f(xi) = n . (Rod(omega) Q + upsilon - c),   Q = (double)q the moved point,   f(0) = the row's d,
    and the row's J must be its gradient at 0.  Central differences with step h: f is linear in upsilon (no truncation) and in omega
    f(h e) - f(-h e) = 2 h J + 2 (h^3 / 6) f''' + ..., |f'''| <= |Q| |n| = |Q|, so the truncation term is h^2 |Q| / 6 (the next one,
    h^4 |Q| / 120, is 1e-9 of it).  Rounding: f is a sum of products of magnitude <= |Q| + |c| + h, each evaluation within
    8 x 2^-53 of that (a 3 x 3 product, a dot product, sin and cos), divided by 2 h and counted twice:
        tol = h^2 |Q| / 6 + 8 x 2^-53 (|Q| + |c| + 1) / h."""
    T = true_pose()
    scan = scan_of(4000, T)
    r = G.rows_ex(room, scan, T, VS, P(VS, cauchy_a=cauchy_a))
    used = r["used"]
    assert used.sum() > 2000
    Q = G.transform(scan, T).astype(np.float64)[used]
    n, c, d, J = r["hits"]["normal"][used], r["hits"]["xyz"][used].astype(np.float64), r["rows"]["d"][used], r["rows"]["J"][used]
    f0 = np.einsum("ij,ij->i", n, Q - c)
    assert np.all(np.abs(f0 - d) <= 4 * EPS * (np.linalg.norm(Q, axis=1) + np.linalg.norm(c, axis=1)))
    h = 1e-4
    nq, nc = np.linalg.norm(Q, axis=1), np.linalg.norm(c, axis=1)
    tol = h * h * nq / 6 + 8 * EPS * (nq + nc + 1) / h
    for a in range(6):
        xi = np.zeros(6)
        xi[a] = h
        fp = np.einsum("ij,ij->i", n, Q @ G.rodrigues(xi[:3]).T + xi[3:] - c)
        fm = np.einsum("ij,ij->i", n, Q @ G.rodrigues(-xi[:3]).T - xi[3:] - c)
        err = np.abs((fp - fm) / (2 * h) - J[:, a])
        assert np.all(err <= tol), (a, float((err / tol).max()))
    # unused points: all-zero rows
    assert not r["rows"][~used].view(np.uint8).any() and not r["rho"][~used].any()
    # k = w2 rho'(s): rho' = 1 without a loss, 1 / (1 + s / a^2) with it
    s = r["w2"][used] * d * d
    rho_p = 1.0 / (1.0 + s / cauchy_a**2) if cauchy_a else np.ones_like(s)
    assert np.allclose(r["rows"]["k"][used], r["w2"][used] * rho_p, rtol=8 * EPS, atol=0)


def test_hand_corner_one_step_recovers_a_translation():
    """The hand map: three faces x, y, z = 0.125 of a corner, 36 dyadic points each (v = 0.5); the planes are exactly the faces (ev[0] = 0,
    the normal a unit axis).  The scan is the map's own points moved by -delta, delta dyadic: at T = identity every point is matched to
    a voxel of its own face and d = -delta_axis exactly.  sigma0 = 2^-4 makes w2 = 256, so every term of H and g is a dyadic number and
    every sum is exact in any order: H equals the sums formed with Fractions, its translation block is 256 x 36 I (36 points per face, each
    seeing exactly one component), and the step solves a consistent system: omega = 0, upsilon = delta."""
    pts, axis = G.hand_corner()
    surf = G.surfels_cpu(pts, G.HAND_V)
    assert len(surf) == 12 and np.all(surf["count"] == 9) and np.all(surf["flags"] == 1) and not surf["ev"][:, 0].any()
    assert sorted(map(tuple, surf["normal"].tolist())) == sorted([(1.0, 0.0, 0.0)] * 4 + [(0.0, 1.0, 0.0)] * 4 + [(0.0, 0.0, 1.0)] * 4)
    delta = np.array([1 / 64, -1 / 32, 1 / 128])
    scan = (pts.astype(np.float64) - delta).astype(np.float32)
    assert np.array_equal(scan.astype(np.float64), pts.astype(np.float64) - delta)  # (dyadic: exact)
    prm = P(G.HAND_V, sigma0=2.0**-4)
    I = np.eye(3, 4)
    r = G.rows_ex(surf, scan, I, G.HAND_V, prm)
    assert r["n_used"] == r["n_found"] == 108
    assert np.array_equal(r["rows"]["d"], -delta[axis]) and np.all(r["rows"]["k"] == 256.0)
    assert np.array_equal(r["rows"]["J"][:, 3:], np.eye(3)[axis])
    H, g, cost, n_used, _ = G.linearize(surf, scan, I, G.HAND_V, prm)
    J = [[Fraction(float(x)) for x in row] for row in r["rows"]["J"]]
    for e, (a, b) in enumerate(G.UPPER):
        assert Fraction(float(H[e])) == sum(256 * j[a] * j[b] for j in J), (a, b)
    for a in range(6):
        assert Fraction(float(g[a])) == sum(256 * j[a] * Fraction(float(d)) for j, d in zip(J, r["rows"]["d"]))
    Hf = G.full(H)
    assert np.array_equal(Hf[3:, 3:], 256.0 * 36 * np.eye(3))
    assert cost == 0.5 * 256 * 36 * float((delta**2).sum())
    xi, piv = G.gn_step(H, g, 1e-9)
    assert min(piv) > 1e-3
    # a consistent system solved by a backward-stable 6 x 6 factorisation: the error is cond x a few ulps; cond <= 1 / min pivot^2 ... held
    # at 1e-12, six orders under delta
    assert np.all(np.abs(xi[:3]) <= 1e-12) and np.all(np.abs(xi[3:] - delta) <= 1e-12), xi
    T1, summ = G.align(surf, scan, I, G.HAND_V, prm, max_iterations=5, tol_rot=1e-9, tol_trans=1e-9)
    assert summ["termination"] == 0 and summ["iterations"] == 2 and summ["final_cost"] <= 1e-20
    assert np.all(np.abs(T1 - np.concatenate([np.eye(3), delta[:, None]], 1)) <= 1e-12)


def test_single_plane_is_refused():
    """one wall: H has rank 3 (the translation across it and the two tilts), a zero diagonal entry makes the scaling non-finite ->
    termination 2, the pose untouched; too few used points likewise"""
    wall = G.hand_wall()
    surf = G.surfels_cpu(wall, G.HAND_V)
    scan = (wall.astype(np.float64) - np.array([0.0, 0.0, 1 / 64])).astype(np.float32)
    T0 = np.eye(3, 4)
    T1, summ = G.align(surf, scan, T0, G.HAND_V, P(G.HAND_V, sigma0=2.0**-4))
    assert summ["termination"] == 2 and summ["iterations"] == 0 and np.array_equal(T1, T0) and summ["n_used"] == 36
    assert summ["initial_cost"] == summ["final_cost"] > 0 and not summ["last_step"].any()
    _, summ = G.align(surf, scan, T0, G.HAND_V, P(G.HAND_V, sigma0=2.0**-4), min_used=37)
    assert summ["termination"] == 2


def test_the_sums_bound_bites(room):
    """the GPU test holds every entry of H and g to (A(n) + 3) x 2^-53 x sum |term| of the longdouble sums.  The float64 sums in the
    device's order meet it; the same sums in float32, or with one tile's partial dropped, miss it"""
    T = true_pose()
    n = 256 * 33 + 7
    scan = scan_of(n, T)
    r = G.rows_ex(room, scan, np.eye(3, 4), VS, P(VS, cauchy_a=0.4))
    ref = G.normal_eq(r["rows"], r["w2"], 0.4)
    J, d, k = r["rows"]["J"], r["rows"]["d"], r["rows"]["k"]
    bound = (G.adds_bound(n) + 3) * EPS
    terms = [(k * J[:, a]) * J[:, b] for a, b in G.UPPER] + [(k * J[:, a]) * d for a in range(6)]
    want = np.concatenate([ref["H"], ref["g"]])
    scale = np.concatenate([ref["absH"], ref["absg"]])
    assert np.all(scale > 0)
    tile = int(np.argmax(np.add.reduceat(r["used"].astype(int), np.arange(0, n, 256))))  # the fullest tile
    for e, t in enumerate(terms):
        assert abs(LD(G.device_order_sum(t)) - want[e]) <= bound * scale[e], e
        assert abs(LD(float(G.device_order_sum(t, np.float32))) - want[e]) > bound * scale[e], (e, "float32")
    # a tile's partial is many orders above the bound in the entries whose terms have one sign (the diagonal of H)
    for e, (a, b) in enumerate(G.UPPER):
        if a == b:
            assert abs(LD(G.device_order_sum(terms[e], drop_tile=tile)) - want[e]) > bound * scale[e], (e, "dropped tile")
    cost = 0.5 * G.device_order_sum(r["rho"])
    assert abs(LD(cost) - ref["cost"]) <= (G.adds_bound(n) + 7) * EPS * ref["abscost"]
    assert abs(LD(0.5 * G.device_order_sum(r["rho"], drop_tile=tile)) - ref["cost"]) > (G.adds_bound(n) + 7) * EPS * ref["abscost"]


def test_restated_alignment_recovers_the_pose(room):
    """the float64 loop on map_surfel_ref's planes, from identity to the issue's pose: convergence, and the last step at least ten
    times under the tolerances the GPU test uses (map_register_ref.TOL_ROT, TOL_TRANS)"""
    T = true_pose()
    scan = scan_of(G.N_ALIGN, T)
    T1, summ = G.align(room, scan, np.eye(3, 4), VS, P(VS), max_iterations=30, tol_rot=G.TOL_ROT, tol_trans=G.TOL_TRANS)
    e_rot, e_tr = G.pose_error(T1, T)
    print("iterations", summ["iterations"], "last step", np.linalg.norm(summ["last_step"][:3]), np.linalg.norm(summ["last_step"][3:]),
          "error", e_rot, e_tr, "cost", summ["initial_cost"], summ["final_cost"], "used", summ["n_used"])
    assert summ["termination"] == 0 and summ["final_cost"] < summ["initial_cost"]
    assert np.linalg.norm(summ["last_step"][:3]) <= G.TOL_ROT / 10 and np.linalg.norm(summ["last_step"][3:]) <= G.TOL_TRANS / 10
    assert e_rot < np.deg2rad(0.1) and e_tr < 0.01  # (from 2 degrees and 6 cm)


def test_header_library_and_records_agree():
    from wildcat_slam_amd import lib

    declared, l = set(lib.declared_symbols()), lib.load()
    for s in ("wc_map_linearize", "wc_map_align"):
        assert s in declared and hasattr(l, s), s
    host = C.CDLL(os.path.join(HERE, "..", "wildcat-slam_amd", "host", "libwildcat_odometry.so"))
    for s in ("wc_odom_map_align", "wc_odom_map_linearize"):
        assert hasattr(host, s), s
    assert _c_fields("wc_map_reg_params") == ["double max_dist", "uint32_t min_points", "uint32_t reserved", "double sigma0", "double cauchy_a"]
    assert [f for f, _ in R.MapRegParams._fields_] == ["max_dist", "min_points", "reserved", "sigma0", "cauchy_a"] and C.sizeof(R.MapRegParams) == 32
    assert _c_fields("wc_map_reg_row") == ["double J[6]", "double d", "double k"]
    assert R.MAP_REG_ROW.itemsize == 64 and [R.MAP_REG_ROW.fields[f][1] for f in ("J", "d", "k")] == [0, 48, 56]
    assert _c_fields("wc_map_normal_eq") == ["double H[21]", "double g[6]", "double cost", "uint64_t n_used", "uint64_t n_found"]
    ne = R.MAP_NORMAL_EQ
    assert ne.itemsize == 240 and [ne.fields[f][1] for f in ("H", "g", "cost", "n_used", "n_found")] == [0, 168, 216, 224, 232]
    assert _c_fields("wc_map_align_opts") == ["wc_map_reg_params reg", "uint32_t max_iterations", "uint32_t min_used", "double tol_rot",
                                              "double tol_trans", "double min_pivot"]
    assert [f for f, _ in R.MapAlignOpts._fields_] == ["reg", "max_iterations", "min_used", "tol_rot", "tol_trans", "min_pivot"]
    assert C.sizeof(R.MapAlignOpts) == 64 and R.MapAlignOpts.tol_rot.offset == 40
    assert _c_fields("wc_map_align_summary") == ["double initial_cost", "double final_cost", "int32_t iterations", "int32_t termination",
                                                 "uint64_t n_used", "uint64_t n_found", "double last_step[6]"]
    assert [f for f, _ in R.MapAlignSummary._fields_] == ["initial_cost", "final_cost", "iterations", "termination", "n_used", "n_found", "last_step"]
    assert C.sizeof(R.MapAlignSummary) == 88 and R.MapAlignSummary.last_step.offset == 40
    assert lib.map_align_opts(lib.map_reg_params(1.0)).min_pivot == 1e-9  # (the default the header names)
