"""Continuous-time registration against the voxel map (include/wildcat_hip.h: wc_map_linearize_ct, wc_map_align_ct) - the parts that need
no GPU: the library's two host entry points against the restatement of map_ct_ref.py byte for byte, the 12 x 12 step by its backward
error, the blended Jacobian against central differences of the true residual (exact at T_begin = T_end, first order otherwise), the blend
against slerp, the recovery of a moving sweep that a rigid registration cannot absorb, and the proof that the GPU test's bound bites."""
import ctypes as C
import os

import numpy as np
import pytest

import map_ct_ref as CT
import map_register_ref as G
from extract_ref import LD
from helpers import xyz_of as _xyz
from test_map_register_ref import P, VS
from test_map_surfel_ref import _c_fields
from wildcat_slam_amd import lib as L
from wildcat_slam_amd import records as R
from wildcat_slam_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = G.EPS
TB, TE = CT.T_BEGIN, CT.T_END
AXIS = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)


def begin_pose():
    """test_map_register_ref's pose as (pos, quat): 2 degrees about (1, 2, 3) / |.|, translation (0.05, -0.03, 0.02) m"""
    return np.array([0.05, -0.03, 0.02]), CT.quat_of_rotvec(np.deg2rad(2.0) * AXIS)


def end_pose(deg=6.0, trans=(0.25, 0.15, -0.05)):
    """the begin pose moved on by `deg` degrees about (1, 2, 3) / |.| and by `trans` (0.296 m): a rotation out of the floor's plane, which a
    rigid registration of the raw sweep cannot absorb (chosen on the CPU: a yaw of the same size mostly slides the points along the room's
    large planes, and the rigid result then stays within the voxel planes' own accuracy)"""
    return CT.pose_update_ct(begin_pose(), np.concatenate([np.deg2rad(deg) * AXIS, np.asarray(trans, np.float64)]))


def start_poses(pb, pe):
    """the perturbed starts of the recovery: 6 to 7 mrad and 2.7 to 3 cm off, in different directions"""
    return (CT.pose_update_ct(pb, np.array([0.004, -0.003, 0.005, 0.02, -0.015, 0.01])),
            CT.pose_update_ct(pe, np.array([-0.005, 0.004, -0.003, -0.02, 0.02, -0.01])))


def sweep_of(n, pb, pe, seed=synth.SEED + 7):
    """a noiseless room scan of n returns measured from the moving sensor -> (body points (m, 3) float32, stamps (m,))"""
    return CT.simulate_sweep(_xyz(synth.g1_room(n, seed=seed, noise=0.0)), pb, pe, TB, TE)


@pytest.fixture(scope="module")
def room():
    return G.surfels_cpu(_xyz(synth.g1_room(200_000)), VS)


def test_interp_move_is_the_restatement_byte_for_byte():
    """wc_pose_interp_move against interp_move: s at 0 and 1, stamps one ulp inside and outside either end, NaN stamps, a flipped end
    quaternion, non-unit quaternions"""
    rng = np.random.Generator(np.random.PCG64(5))
    n = 1000
    xyz = (30 * rng.normal(size=(n, 3))).astype(np.float32)
    t = np.sort(rng.uniform(TB, TE, n))
    t[:8] = [TB, TE, np.nextafter(TB, np.inf), np.nextafter(TB, -np.inf), np.nextafter(TE, -np.inf), np.nextafter(TE, np.inf), np.nan, -np.nan]
    t[8:12] = [np.inf, -np.inf, 0.0, 0.5 * (TB + TE)]
    pb, pe = begin_pose(), end_pose()
    cases = [(pb, pe), (pb, (pe[0], -pe[1])), ((pb[0], 3.0 * pb[1]), (pe[0], 3.0 * pe[1])), ((pb[0], -0.7 * pb[1]), (pe[0], -0.7 * pe[1])),
             (pb, pb), ((pb[0], 3.0 * pb[1]), (pe[0], 0.25 * pe[1])), ((rng.normal(size=3), rng.normal(size=4)), (rng.normal(size=3), rng.normal(size=4)))]
    outs = []
    for b, e in cases:
        want, s, inside = CT.interp_move(b, e, TB, TE, xyz, t)
        got = L.pose_interp_move(b, e, TB, TE, xyz, t)
        assert got.tobytes() == want.tobytes()
        assert list(inside[:12]) == [True, True, True, False, True, False, False, False, False, False, False, True]
        assert np.isnan(got[~inside]).all() and np.isfinite(got[inside]).all()
        assert s[0] == 0.0 and s[1] == 1.0 and abs(s[11] - 0.5) < 1e-11
        outs.append(got)
    assert outs[0].tobytes() == outs[1].tobytes()  # (the flipped end quaternion is the same rotation: the host negates it back)
    # s = 0 and s = 1 are the rigid moves by the end poses: against map_register_ref.transform to float rounding
    for j, p in ((0, pb), (1, pe)):
        assert np.allclose(outs[0][j], G.transform(xyz[j : j + 1], CT.pose_T(p))[0], rtol=0, atol=2.0**-22 * 60)
    # quaternions of a common norm other than 1 give the unit ones' points up to rounding, not bitwise (norms that differ weigh the blend)
    assert np.allclose(outs[2][inside], outs[0][inside], rtol=0, atol=1e-4) and np.allclose(outs[3][inside], outs[0][inside], rtol=0, atol=1e-4)
    lib = L.load()
    out = np.zeros((n, 3), np.float32)

    def rc(b=pb, e=pe, tb=TB, te=TE):
        bb, ee = L._pose_rec(b), L._pose_rec(e)
        return lib.wc_pose_interp_move(C.byref(bb), C.byref(ee), C.c_double(tb), C.c_double(te), R.ptr(xyz), R.ptr(t), C.c_uint64(n), R.ptr(out))

    assert rc() == 0
    for kw in (dict(te=TB), dict(te=TB - 1), dict(tb=np.nan), dict(te=np.inf), dict(b=(pb[0], np.zeros(4))), dict(e=(pe[0], np.zeros(4))),
               dict(b=(np.array([np.nan, 0, 0]), pb[1])), dict(e=(pe[0], np.array([1, np.inf, 0, 0])))):
        assert rc(**kw) == 11, kw
    assert lib.wc_pose_interp_move(None, None, C.c_double(TB), C.c_double(TE), None, None, C.c_uint64(0), None) == 11


def _random_record(rng, n=400):
    """a MAP_CT_NORMAL_EQ record of n random rows (numpy's own sums: only the record matters here)"""
    rows = np.zeros(n, R.MAP_CT_ROW)
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    Q = 20 * rng.normal(size=(n, 3))
    rows["J"] = np.concatenate([np.cross(Q, nrm), nrm], 1)
    rows["d"], rows["k"], rows["s"] = 0.05 * rng.normal(size=n), rng.uniform(100, 14000, n), rng.uniform(0, 1, n)
    ne = np.zeros(1, R.MAP_CT_NORMAL_EQ)[0]
    for name, val in CT._split([x.sum() for x in CT.terms_ct(rows)]).items():
        ne[name] = val
    return ne


@pytest.mark.parametrize("prior", [(0.0, 0.0, 0.0, 0.0), (10.0, 100.0, 5.0, 50.0), (1e30, 1e30, 0.0, 0.0)])
def test_step12(prior):
    """wc_map_ct_step against step12 byte for byte, and against the exact system by its backward error, as test_map_register_gpu's
    test_one_step does for 6 x 6 with the sums' error beta = 0 (the record is the input here):
      scaling    D~_a = fl(1 / fl(sqrt(A_aa))): relative error 2u; A~_ab = fl(fl(D~_a A_ab) D~_b), the diagonal exactly 1: |A~_ab - S_ab| <= 6u off
                 the diagonal (|S_ab| <= 1), 132 entries: |A~ - S|_2 <= sqrt(132) 6u;  b~_a = fl(D~_a b_a): |b~ - c|_2 <= 3u |c|_2
      Cholesky   Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Theorem 10.4: (A~ + dA) y^ = b~, |dA| <= gamma_(3n+1) |R^T| |R|,
                 and (10.7) | |R^T| |R| |_2 <= n (1 - n gamma_(n+1))^-1 |A~|_2: with n = 12, |dA|_2 <= 12 gamma_37 / (1 - 12 gamma_13) |A~|_2
      unscaling  y = D^-1 xi^ = y^ (1 + e), |e| <= 3u
    so |S y - c|_2 <= [sqrt(132) 6u + (12 gamma_37 / (1 - 12 gamma_13) + 3u) |S|_2] |y|_2 + 3u |c|_2, times 1.01 for the second-order terms; S, c:
    the unit-diagonal system in longdouble.  numpy.linalg.solve of the same system then differs from y by at most |S^-1|_2 times the two
    residuals.  A begin prior of 1e30 leaves the begin pose where it is: its step is below 1e-20."""
    rng = np.random.Generator(np.random.PCG64(11))
    ne = _random_record(rng)
    acc = 1e-3 * rng.normal(size=12)
    if prior[0] >= 1e30:
        acc[:6] = 0  # (the loop's own state under such a prior: no step has moved the begin pose)
    want = CT.step12(ne, prior, acc, 1e-9)
    got = L.map_ct_step(ne, prior, acc, 1e-9)
    assert want is not None and got.tobytes() == want.tobytes()
    A, b = CT.full12(ne, prior, acc, LD)
    D = 1 / np.sqrt(np.diag(A))
    S, c = A * D[:, None] * D[None, :], -(D * b)
    y = got.astype(LD) / D
    u = LD(EPS)
    gam = lambda k: k * u / (1 - k * u)  # noqa: E731
    norm2 = lambda x: np.sqrt((x * x).sum())  # noqa: E731
    S64 = S.astype(np.float64)
    normS = LD(np.linalg.norm(S64, 2)) * (1 + 1e-12)
    bound = ((np.sqrt(LD(132)) * 6 * u + (12 * gam(37) / (1 - 12 * gam(13)) + 3 * u) * normS) * norm2(y) + 3 * u * norm2(c)) * LD(1.01)
    res = norm2(S @ y - c)
    print("step12: |S y - c| / bound =", float(res / bound), "|S|_2 =", float(normS), "cond =", float(np.linalg.cond(S64)))
    assert res <= bound
    y_np = np.linalg.solve(S64, c.astype(np.float64)).astype(LD)
    inv_norm = LD(np.linalg.norm(np.linalg.inv(S64), 2)) * (1 + 1e-6)
    assert norm2(y - y_np) <= inv_norm * (bound + norm2(S @ y_np - c))
    if prior[0] >= 1e30:
        assert np.all(np.abs(got[:6]) <= 1e-20) and np.abs(got[6:]).max() > 1e-6
    # refusals and a rank-deficient system
    lib = L.load()
    xi = np.full(12, 7.0)
    pr, ac, rec = np.zeros(4), np.zeros(12), np.ascontiguousarray(ne).reshape(1)
    assert lib.wc_map_ct_step(R.ptr(rec), R.ptr(pr), R.ptr(ac), C.c_double(0.0), R.ptr(xi)) == 11
    assert lib.wc_map_ct_step(R.ptr(rec), R.ptr(np.array([0, -1.0, 0, 0])), R.ptr(ac), C.c_double(1e-9), R.ptr(xi)) == 11
    assert lib.wc_map_ct_step(None, R.ptr(pr), R.ptr(ac), C.c_double(1e-9), R.ptr(xi)) == 11
    flat = rec.copy()
    flat["H11"], flat["H01"], flat["g1"] = 0, 0, 0  # every stamp at t_begin: the end pose is free
    assert L.map_ct_step(flat[0]) is None and CT.step12(flat[0]) is None and np.all(xi == 7.0)
    assert L.map_ct_step(flat[0], (0, 0, 1.0, 1.0)) is not None  # ... and the prior holds it


def _true_moved(pb, pe, s, p):
    """the model's moved points in float64, no float cast: R(s) p + c(s) with the normalised blend"""
    p0, q0, p1, q1 = CT.host_poses(pb, pe)
    q = (1.0 - s)[:, None] * q0 + s[:, None] * q1
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    c = (1.0 - s)[:, None] * p0 + s[:, None] * p1
    u = np.cross(q[:, 1:], p)
    return p + 2.0 * (q[:, 0:1] * u + np.cross(q[:, 1:], u)) + c


def _jacobian_errors(room, pb, pe, n=4000, h=1e-4):
    """central differences of the true residual on FIXED planes against the blended rows -> per used point and per entry of xi (12):
    |fd - a J_i| or |fd - s J_i|, the finite-difference tolerance, and a, s, |p|"""
    body, times = sweep_of(n, pb, pe)
    r = CT.rows_ct(room, body, times, pb, pe, TB, TE, VS, P(VS))
    used = r["used"]
    assert used.sum() > n // 2
    p = body.astype(np.float64)[used]
    s = r["rows"]["s"][used]
    nrm, J = r["rows"]["J"][used][:, 3:], r["rows"]["J"][used]

    def f(xi):
        return np.einsum("ij,ij->i", nrm, _true_moved(CT.pose_update_ct(pb, xi[:6]), CT.pose_update_ct(pe, xi[6:]), s, p))

    err = np.zeros((used.sum(), 12))
    for a in range(12):
        xi = np.zeros(12)
        xi[a] = h
        fd = (f(xi) - f(-xi)) / (2 * h)
        share = (1.0 - s) if a < 6 else s
        err[:, a] = np.abs(fd - share * J[:, a % 6])
    npn = np.linalg.norm(p, axis=1)
    P0 = _true_moved(pb, pe, s, p)
    nP = np.linalg.norm(P0, axis=1)
    cmax = max(np.linalg.norm(pb[0]), np.linalg.norm(pe[0]))
    # truncation: f is odd-differenced, |f'''| <= 1.03 |p| + |pos| (the blend's angle is theta(h) = a h + c3 h^3, |c3| <= 0.005 a, on top of
    # the rotation's own third derivative |p|; the lever arm of the pose's own position adds |pos|); rounding: 24 operations of magnitude
    # <= |P| + 1 per evaluation, divided by 2 h and counted twice; the float cast: J is formed at Q = (float)P, |Q - P| <= 2^-24 |P|
    tol = h * h * (1.03 * npn + cmax) / 6 + 24 * EPS * (nP + 1) / h + 2.0**-24 * nP
    return err, tol, 1.0 - s, s, npn


def test_blended_jacobian_is_exact_where_the_poses_agree(room):
    """T_begin = T_end: d(dist) = a J . xi_begin + s J . xi_end holds to the central differences' own tolerance (the truncation-derived one
    of test_map_register_ref, with the float cast of the moved point added: the true residual here is formed without it)"""
    pb = begin_pose()
    err, tol, a, s, _ = _jacobian_errors(room, pb, pb)
    ratio = err / tol[:, None]
    print("static: max err / tol =", float(ratio.max()))
    assert np.all(ratio <= 1.0)
    assert a.min() < 0.01 and s.min() < 0.01  # (both ends of the sweep are there)


def test_blended_jacobian_is_first_order_in_the_motion(room):
    """0.3 m and 6 degrees between the poses: an entry of the gradient with respect to omega_begin differs from a J_i by at most
    a (s D + (phi + phi^2 / 2) |p|), with respect to omega_end by at most s (a D + (phi + phi^2 / 2) |p|), D = |p_end - p_begin|, phi =
    Theta / 2 the angle between the two quaternions; the upsilon entries are exact.
    Derivation (the header's): the position blends linearly, dc / d omega_begin = -a [p_begin]x where the model takes -a [c(s)]x: the
    difference is a s [p_end - p_begin]x, at most a s D on a unit normal.  The rotation: q(s) ~ (N + a (0, omega / 2) r) q^(s), r the unit
    quaternion from q^(s) to q_begin (angle alpha <= phi), N = |a q_begin + s q_end| in [cos(phi / 2), 1]; its rotation vector is
    (a / N) (cos(alpha) omega + sin(alpha) omega x axis) where the model takes a omega: |cos(alpha) / N - 1| <= phi^2 / 2 and
    sin(alpha) / N <= sin(phi) / cos(phi / 2) <= phi, times the lever arm |p|.
    The bound bites: a tenth of it is missed by a clear share of the entries."""
    pb, pe = begin_pose(), end_pose()
    err, tol, a, s, npn = _jacobian_errors(room, pb, pe)
    theta, D = CT.pose_error(pe, pb)
    phi = 0.5 * theta
    lever = (phi + 0.5 * phi * phi) * npn
    bound = np.zeros_like(err)
    bound[:, 0:3] = (a * (s * D + lever))[:, None]
    bound[:, 6:9] = (s * (a * D + lever))[:, None]
    ratio = err / (bound + tol[:, None])
    rot = [0, 1, 2, 6, 7, 8]
    print("moving: max err / (bound + tol) =", float(ratio.max()), "rotation entries over a tenth of the bound:",
          float((err[:, rot] > bound[:, rot] / 10 + tol[:, None]).mean()))
    assert np.all(ratio <= 1.0)
    assert np.all(err[:, [3, 4, 5, 9, 10, 11]] <= tol[:, None])  # (upsilon: exact)
    assert (err[:, rot] > bound[:, rot] / 10 + tol[:, None]).mean() > 0.05
    assert ratio[:, rot].max() > 0.3


@pytest.mark.parametrize("theta", [0.01, 0.05, 0.1, 0.2])
def test_blend_against_slerp(theta):
    """the angle between the blend's rotation and slerp's at the same s equals the closed form
    2 atan2(s sin(Theta / 2), (1 - s) + s cos(Theta / 2)) - s Theta; extremal near s = 0.21 and 0.79 at about 0.004 Theta^3"""
    q0 = CT.quat_of_rotvec(np.array([0.3, -0.2, 0.1]))
    q1 = CT.quat_mul(CT.quat_of_rotvec(theta * AXIS), q0)
    s = np.linspace(0, 1, 101)
    got = np.zeros_like(s)
    for j, sj in enumerate(s):
        qb = ((1 - sj) * q0 + sj * q1).astype(LD)
        qs = CT.quat_mul(CT.quat_of_rotvec(sj * theta * AXIS), q0).astype(LD)
        qb, qs = qb / np.sqrt((qb * qb).sum()), qs / np.sqrt((qs * qs).sum())
        # the rotation from slerp's to the blend's: qb qs^-1, its signed angle about AXIS
        w = (qb * qs).sum()
        v = qs[0] * qb[1:] - qb[0] * qs[1:] - np.cross(qb[1:].astype(np.float64), qs[1:].astype(np.float64)).astype(LD)
        got[j] = float(2 * np.arctan2((v * AXIS.astype(LD)).sum(), w))
    want = CT.blend_minus_slerp(theta, s)
    assert np.all(np.abs(got - want) <= 64 * EPS), float(np.abs(got - want).max())
    assert want[0] == 0 and abs(want[50]) <= 4 * EPS and abs(want[100]) <= 4 * EPS
    peak = np.abs(want).max()
    assert s[np.argmax(np.abs(want))] in (0.21, 0.79) and abs(peak / theta**3 - 0.00401) <= 2e-5
    if theta == 0.2:
        assert abs(peak - 3.2e-5) <= 1e-6  # (DESIGN 8.12's value)
    # the library's own move follows the closed form: a unit vector across the axis, turned by wc_pose_interp_move between (0, q0) and (0, q1),
    # makes the angle s Theta + delta(s) with its image under q0, to the float cast of the moved point (2^-24 per component of a unit
    # vector, sqrt(3) of them, and as much again for the reference image: 4 x 2^-24 on the angle)
    e = np.cross(AXIS, [1.0, 0.0, 0.0])
    e /= np.linalg.norm(e)
    p = (CT.quat_rot(q0).T @ e).astype(np.float32)  # (q0 takes it to e, up to the cast)
    zero = np.zeros(3)
    moved = L.pose_interp_move((zero, q0), (zero, q1), 0.0, 1.0, np.repeat(p[None], len(s), 0), s).astype(np.float64)
    at0 = moved[0]
    ang = np.arctan2(np.cross(at0, moved) @ AXIS, moved @ at0)
    assert np.all(np.abs(ang - (s * theta + want)) <= 4 * 2.0**-24), float(np.abs(ang - (s * theta + want)).max())


def test_restated_alignment_recovers_a_moving_sweep(room):
    """A sweep measured while the sensor moves 0.3 m and 6 degrees (end_pose), from starts 3 cm and 7 mrad off: the continuous-time loop ends
    at the truth to what the voxel planes allow - the same 0.2 to 0.5 mrad and 4 to 5 mm at which the rigid loop ends on a sweep measured
    at rest (below) -, and the rigid registration of the same raw sweep ends measurably further from the sweep's midpoint pose than the
    continuous-time one is from the truth at the begin, the midpoint and the end."""
    pb, pe = begin_pose(), end_pose()
    body, times = sweep_of(CT.N_SWEEP, pb, pe)
    pb0, pe0 = start_poses(pb, pe)
    kw = dict(max_iterations=30, tol_rot=CT.TOL_ROT, tol_trans=CT.TOL_TRANS)
    b1, e1, summ = CT.align_ct(room, body, times, pb0, pe0, TB, TE, VS, P(VS), **kw)
    mid = CT.blend_pose(pb, pe, 0.5)
    errs = [CT.pose_error(b1, pb), CT.pose_error(CT.blend_pose(b1, e1, 0.5), mid), CT.pose_error(e1, pe)]
    T_rigid, s_rigid = G.align(room, body, CT.pose_T(CT.blend_pose(pb0, pe0, 0.5)), VS, P(VS), **kw)
    e_rigid = G.pose_error(T_rigid, CT.pose_T(mid))
    still, _ = sweep_of(CT.N_SWEEP, pb, pb)
    T_still, s_still = G.align(room, still, CT.pose_T(pb0), VS, P(VS), **kw)
    e_still = G.pose_error(T_still, CT.pose_T(pb))
    print("continuous time:", errs, "iterations", summ["iterations"], "used", summ["n_used"], "rigid:", e_rigid, s_rigid["iterations"],
          "at rest:", e_still, "last step", summ["last_step"])
    assert summ["termination"] == 0 and s_rigid["termination"] == 0 and s_still["termination"] == 0
    assert summ["final_cost"] < summ["initial_cost"] and summ["n_used"] > 0.95 * len(body) and summ["n_outside"] == 0
    for e_rot, e_tr in errs:
        # the voxel planes' own accuracy is what the rigid loop reaches at rest; two poses share the sweep's points, each is held by about
        # half of them: sqrt(2) of that error, taken as 2
        assert e_rot <= 2 * e_still[0] and e_tr <= 2 * e_still[1]
        assert e_rot < e_rigid[0] and e_tr < e_rigid[1]  # the issue's condition
    assert e_rigid[0] > 2 * e_still[0] and e_rigid[1] > 2 * e_still[1]  # the rigid result is outside that accuracy: the motion is not absorbed


def test_the_sums_bound_bites(room):
    """the GPU test holds each of the 75 weighted sums to (A(n) + 6) x 2^-53 x sum |term| of the longdouble sums (map_ct_ref.SUM_C).  The
    float64 sums in the device's order meet it; the same sums in float32, or with one tile's partial dropped, miss it"""
    pb, pe = begin_pose(), end_pose()
    n = 256 * 33 + 7
    body, times = sweep_of(n + 200, pb, pe)
    body, times = body[:n], times[:n]
    assert len(body) == n
    r = CT.rows_ct(room, body, times, pb, pe, TB, TE, VS, P(VS, cauchy_a=0.4))
    ref = CT.normal_eq_ct(r["rows"], r["w2"], 0.4)
    bound = (G.adds_bound(n) + CT.SUM_C) * EPS
    terms = CT.terms_ct(r["rows"])
    want = np.concatenate([ref[k] for k, _ in CT.NAMES])
    scale = np.concatenate([ref["abs" + k] for k, _ in CT.NAMES])
    assert len(terms) == 75 and np.all(scale > 0)
    tile = int(np.argmax(np.add.reduceat(r["used"].astype(int), np.arange(0, n, 256))[1:-1])) + 1  # the fullest tile inside the sweep
    diag = [e for blk in range(3) for e, (a, b) in enumerate(G.UPPER, 21 * blk) if a == b]
    for e, t in enumerate(terms):
        assert abs(LD(G.device_order_sum(t)) - want[e]) <= bound * scale[e], e
        assert abs(LD(float(G.device_order_sum(t, np.float32))) - want[e]) > bound * scale[e], (e, "float32")
    for e in diag:  # (terms of one sign: a tile's partial is many orders above the bound)
        assert abs(LD(G.device_order_sum(terms[e], drop_tile=tile)) - want[e]) > bound * scale[e], (e, "dropped tile")
    cost = 0.5 * G.device_order_sum(r["rho"])
    assert abs(LD(cost) - ref["cost"]) <= (G.adds_bound(n) + 7) * EPS * ref["abscost"]
    assert abs(LD(0.5 * G.device_order_sum(r["rho"], drop_tile=tile)) - ref["cost"]) > (G.adds_bound(n) + 7) * EPS * ref["abscost"]


def test_header_library_and_records_agree():
    declared, l = set(L.declared_symbols()), L.load()
    for s in ("wc_map_linearize_ct", "wc_map_align_ct", "wc_pose_interp_move", "wc_map_ct_step"):
        assert s in declared and hasattr(l, s), s
    host = C.CDLL(os.path.join(HERE, "..", "wildcat-slam_amd", "host", "libwildcat_odometry.so"))
    assert hasattr(host, "wc_odom_map_align_sweep")
    assert _c_fields("wc_map_ct_normal_eq") == ["double H00[21]", "double H01[21]", "double H11[21]", "double g0[6]", "double g1[6]", "double cost",
                                                "uint64_t n_used", "uint64_t n_found", "uint64_t n_outside", "uint64_t reserved"]
    ne = R.MAP_CT_NORMAL_EQ
    assert ne.itemsize == 640
    assert [ne.fields[f][1] for f in ("H00", "H01", "H11", "g0", "g1", "cost", "n_used", "n_found", "n_outside", "reserved")] == [
        0, 168, 336, 504, 552, 600, 608, 616, 624, 632]
    assert _c_fields("wc_map_ct_row") == ["double J[6]", "double d", "double k", "double s"]
    assert R.MAP_CT_ROW.itemsize == 72 and [R.MAP_CT_ROW.fields[f][1] for f in ("J", "d", "k", "s")] == [0, 48, 56, 64]
    assert _c_fields("wc_map_ct_align_opts") == ["wc_map_reg_params reg", "uint32_t max_iterations", "uint32_t min_used", "double tol_rot",
                                                 "double tol_trans", "double min_pivot", "double prior[4]"]
    assert [f for f, _ in R.MapCtAlignOpts._fields_] == ["reg", "max_iterations", "min_used", "tol_rot", "tol_trans", "min_pivot", "prior"]
    assert C.sizeof(R.MapCtAlignOpts) == 96 and R.MapCtAlignOpts.prior.offset == 64
    assert _c_fields("wc_map_ct_align_summary") == ["double initial_cost", "double final_cost", "int32_t iterations", "int32_t termination",
                                                    "uint64_t n_used", "uint64_t n_found", "uint64_t n_outside", "double last_step[12]",
                                                    "double prior_cost"]
    assert [f for f, _ in R.MapCtAlignSummary._fields_] == ["initial_cost", "final_cost", "iterations", "termination", "n_used", "n_found",
                                                            "n_outside", "last_step", "prior_cost"]
    assert C.sizeof(R.MapCtAlignSummary) == 152 and R.MapCtAlignSummary.last_step.offset == 48 and R.MapCtAlignSummary.prior_cost.offset == 144
    assert C.sizeof(R.Pose) == 56 == R.POSE.itemsize
    o = L.map_ct_align_opts(L.map_reg_params(1.0))
    assert o.min_pivot == 1e-9 and o.min_used == 12 and list(o.prior) == [0.0] * 4
