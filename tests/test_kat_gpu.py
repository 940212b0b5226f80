"""The reference's SO(3) known-answer tests (src/common/utils_test.cc:5-21) against the DEVICE instantiation of
csrc/dmath.h — the code the kernels run — through the C-ABI self-test entry points."""
import ctypes as C

import numpy as np
import pytest

from test_host_kat import check_so3_kats, unpack_so3
from wildcat_slam_amd import records as R

pytestmark = pytest.mark.gpu


def so3_device(gpu, v):
    out = np.zeros(52)
    gpu._ck(gpu.lib.wc_selftest_so3(gpu.h, R.ptr(np.ascontiguousarray(v, float)), C.c_int(1), R.ptr(out)))
    return unpack_so3(out)


def test_dmath_so3_kats_on_the_device(gpu):
    check_so3_kats(lambda v: so3_device(gpu, v))


def test_device_and_host_instantiations_agree(gpu, oracle):
    rng = np.random.default_rng(11)
    for _ in range(30):
        v = rng.normal(size=3) * rng.choice([1e-11, 1e-2, 1.0])
        d = so3_device(gpu, v)
        out = np.zeros(52)
        assert gpu.lib.wc_selftest_so3(C.c_void_p(0), R.ptr(np.ascontiguousarray(v)), C.c_int(0), R.ptr(out)) == 0
        h = unpack_so3(out)
        for k in d:  # device libm (ocml) vs glibc: a few ulp
            assert np.allclose(d[k], h[k], rtol=0, atol=8e-16 * max(1.0, np.abs(h[k]).max())), k
        assert np.allclose(d["jl"], oracle.so3_jl(v), atol=1e-14)


def test_eig3_and_quaternions_on_the_device(gpu):
    rng = np.random.default_rng(4)
    for _ in range(100):
        a = rng.normal(size=(3, 3))
        a = a @ a.T * 10 ** rng.uniform(-6, 2)
        out = np.zeros(12)
        gpu._ck(gpu.lib.wc_selftest_eig3(gpu.h, R.ptr(np.ascontiguousarray(a)), C.c_int(1), R.ptr(out)))
        ev, v = out[:3], out[3:].reshape(3, 3)
        ev2 = np.linalg.eigvalsh(a)
        assert np.abs(ev - ev2).max() <= 4e-15 * ev2.max()
        assert np.abs(a @ v - v * ev).max() <= 1e-14 * ev2.max()
    for _ in range(50):
        qa, qb = rng.normal(size=4), rng.normal(size=4)
        qa, qb = qa / np.linalg.norm(qa), qb / np.linalg.norm(qb)
        f, p = rng.uniform(), rng.normal(size=3)
        inp = np.concatenate([qa, qb, [f], p])
        od, oh = np.zeros(11), np.zeros(11)
        gpu._ck(gpu.lib.wc_selftest_quat(gpu.h, R.ptr(inp), C.c_int(1), R.ptr(od)))
        assert gpu.lib.wc_selftest_quat(C.c_void_p(0), R.ptr(inp), C.c_int(0), R.ptr(oh)) == 0
        assert np.allclose(od, oh, atol=1e-15)
        # slerp end points and unit rotation
        w, x, y, z = qa
        Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                       [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        assert np.allclose(od[4:7], Rm @ p, atol=1e-14)


def test_fused_so3_forms_of_the_factor_kernels(gpu):
    """csrc/so3_fused.h (Exp + Jr from one sincos, Jr^-1 of a logarithm from the quaternion: what k_lin_imu / k_eval_imu
    evaluate instead of cost_functor.h:286-321's separate calls) against the dmath.h helpers the reference's KATs pin,
    on the device, from the series branch (|v| < 1e-10) to rotations close to pi.  The Jr^-1 coefficient 1 - th cot(th/2) / 2
    cancels for small th in BOTH forms (utils.h:38), hence the absolute tolerance on it."""
    rng = np.random.default_rng(23)
    vs = [np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0) * 3.0, np.zeros(3), np.array([3.1, 0.0, 0.0])]
    vs += [rng.normal(size=3) * s for s in (1e-12, 1e-9, 1e-6, 1e-3, 0.1, 1.0) for _ in range(8)]
    for v in vs:
        n = np.linalg.norm(v)
        if n > 3.1:
            v = v * (3.1 / n)
        d = so3_device(gpu, v)
        out = np.zeros(25)
        gpu._ck(gpu.lib.wc_selftest_so3_fused(gpu.h, R.ptr(np.ascontiguousarray(v, float)), R.ptr(out)))
        assert np.allclose(out[0:4], d["exp"], rtol=0, atol=4e-16), v
        # (utils.h:52 forms (1 - cos th) / th: zero below th = 1.5e-8 and ~1e-16 / th of rounding noise above; the fused form
        # 2 sin^2(th / 2) / th has neither, so the two differ by exactly that)
        assert np.allclose(out[4:13].reshape(3, 3), d["jr"], rtol=0, atol=2e-15 + (min(0.5 * n, 4e-16 / n) if n > 0 else 0.0)), v
        assert np.allclose(out[13:16], d["log_exp"], rtol=0, atol=1e-15 * max(1.0, n)), v
        assert np.allclose(out[16:25].reshape(3, 3), d["jr_inv"], rtol=0, atol=1e-9), v
        # Jr_inv(v) Jr(v) = I (utils_test.cc:5-12 with v -> -v)
        assert np.allclose(out[16:25].reshape(3, 3) @ out[4:13].reshape(3, 3), np.eye(3), atol=1e-9), v


def test_diagonal_block_factor_and_inverse(gpu):
    """the damped solve's 32 x 32 diagonal-block kernel on its own (csrc/window.hip: factor_inv32_blk, the critical path of every panel
    step): L and L^-1 of random SPD matrices against numpy, and a matrix that is not positive definite is reported"""
    rng = np.random.default_rng(5)
    for trial in range(4):
        b = rng.normal(size=(32, 40))
        a = b @ b.T + (1e-3 if trial == 0 else 0.5) * np.eye(32)
        L, X, clk, ok = gpu.selftest_factor32(a, 0, 2)
        Lr = np.linalg.cholesky(a)
        Xr = np.linalg.inv(Lr)
        assert ok and clk > 0
        assert np.abs(np.tril(L) - Lr).max() <= 1e-13 * np.abs(Lr).max()
        assert np.abs(np.tril(X) - Xr).max() <= 1e-12 * np.abs(Xr).max()
    assert not gpu.selftest_factor32(-np.eye(32), 0, 1)[3]


# ---- fx_eig3: the closed-form eigen-solver behind every surfel of the default extraction path ------------------------------------------
def _rot(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q


def _sym(q, lam):
    a = (q * np.asarray(lam, float)) @ q.T
    return (a + a.T) / 2


def _fx_eig3_cases():
    """(family, matrix): what extraction hands to fx_eig3 and what could break it.  The matrices are whatever fp64 made of the recipe; the
    reference decomposes exactly those (extract_ref.jacobi_eigh, longdouble)."""
    rng = np.random.default_rng(41)
    cases = []
    for k in range(15):  # plane-like: lambda_0 / lambda_2 from 1 down to 1e-14, overall scales 1e-8 .. 1e2
        for _ in range(10):
            r, scale = 10.0**-k, 10 ** rng.uniform(-8, 2)
            cases.append(("plane", _sym(_rot(rng), [r * scale, scale * rng.uniform(max(r, 0.3), 1.0), scale])))
    for _ in range(30):  # exactly rank 2, from small-integer vectors: lambda_0 = 0
        u, w = rng.integers(-5, 6, size=3).astype(float), rng.integers(-5, 6, size=3).astype(float)
        if np.linalg.norm(np.cross(u, w)) > 0:
            cases.append(("rank2", (np.outer(u, u) + np.outer(w, w)) * 2.0 ** int(rng.integers(-20, 4))))
    perms = [np.eye(3)[list(p)] * np.array(s)[:, None] for p in ((0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1)) for s in ((1, 1, 1), (-1, 1, -1))]
    for i, pm in enumerate(perms):  # two equal eigenvalues, exactly: diagonal, rotated by a signed permutation (stays diagonal)
        cases.append(("equal12_exact", pm @ np.diag([0.001 * (i + 1), 0.5, 0.5]) @ pm.T))
        cases.append(("equal01_exact", pm @ np.diag([0.25, 0.25, 3.0 + i]) @ pm.T))
    for _ in range(12):  # ... and within 1e-12, in general position
        scale = 10 ** rng.uniform(-8, 2)
        cases.append(("equal12_near", _sym(_rot(rng), [scale * 10 ** rng.uniform(-6, -1), scale, scale * (1 + 1e-12)])))
        cases.append(("equal01_near", _sym(_rot(rng), [scale * 0.01, scale * 0.01 * (1 + 1e-12), scale])))
    for _ in range(6):  # all three equal: exactly (diagonal), and as a rotation's rounding leaves it
        scale = 10 ** rng.uniform(-8, 2)
        cases.append(("equal_all", np.eye(3) * scale))
        cases.append(("equal_all", _sym(_rot(rng), [scale, scale, scale])))
    for _ in range(10):  # diagonal: p1 == 0, the fall-back by construction
        cases.append(("diagonal", np.diag(10 ** rng.uniform(-8, 2, size=3))))
    for i in range(12):  # axis-aligned planes with off-diagonals of 1e-20
        d = np.roll([10 ** rng.uniform(-9, -5), 0.004 * rng.uniform(0.5, 1), 0.006], i)
        cases.append(("axis_plane", np.diag(d) + 1e-20 * (np.ones((3, 3)) - np.eye(3)) * rng.choice([-1.0, 1.0])))
    for _ in range(24):  # a smallest eigenvalue slightly below zero, as rounded covariances of exactly planar clusters have
        scale = 10 ** rng.uniform(-8, 2)
        cases.append(("negative", _sym(_rot(rng), [-scale * 10 ** rng.uniform(-17, -13), scale * rng.uniform(0.2, 1), scale])))
    return cases


def test_fx_eig3_against_longdouble_jacobi(gpu):
    """wc_selftest_fx_eig3 (one thread, the routine fx_pca calls) on ~300 matrices against the longdouble Jacobi iteration of
    tests/extract_ref.py: eigenvalues ascending and within 32 x 2^-53 of the largest magnitude; unit eigenvector; residual
    |(A - lambda_0 I) v| <= 1e-12 (|lambda_0| + |lambda_2|), the bar at which the routine accepts its own result; where lambda_1 - lambda_0 >
    1e-6 lambda_2 the vector within (32 x 2^-53 lambda_2 + 1e-12 (|lambda_0| + lambda_2)) / (lambda_1 - lambda_0) of the reference's (the
    surfel bound of test_extract_precision_gpu.py with B_cov = 0); and the closed form ACCEPTED on every plane-like matrix whose likeness
    exceeds 0.1 unless it is diagonal (p1 == 0 goes to the Jacobi iteration by construction) - those must not quietly run on the slow path."""
    import extract_ref as X

    cases = _fx_eig3_cases()
    assert 250 <= len(cases) <= 400
    A = np.array([c[1] for c in cases])
    ev_ref, V_ref = X.jacobi_eigh(A)
    worst = {}
    fails = []
    for i, (fam, a) in enumerate(cases):
        ev, v, accepted = gpu.selftest_fx_eig3(a)
        lr = ev_ref[i].astype(np.float64)
        scale = np.abs(lr).max()
        al, vl = a.astype(X.LD), v.astype(X.LD)
        r_ev = float(np.abs(ev.astype(X.LD) - ev_ref[i]).max()) / (32 * 2.0**-53 * scale)
        r_unit = abs(float(np.sqrt((vl * vl).sum()) - 1)) / (8 * 2.0**-53)
        r_res = float(np.sqrt((((al - X.LD(ev[0]) * np.eye(3)) @ vl) ** 2).sum())) / (1e-12 * (abs(ev[0]) + abs(ev[2])))
        r_vec = 0.0
        if lr[1] - lr[0] > 1e-6 * lr[2]:
            vr = V_ref[i][:, 0]
            sgn = -1 if float((vl * vr).sum()) < 0 else 1
            r_vec = float(np.sqrt(((sgn * vl - vr) ** 2).sum())) / ((32 * 2.0**-53 * lr[2] + 1e-12 * (abs(lr[0]) + lr[2])) / (lr[1] - lr[0]))
        like = 2 * (lr[1] - lr[0]) / lr.sum()
        diagonal = not np.any(a - np.diag(np.diag(a)))
        must_accept = like > 0.1 and not diagonal and fam in ("plane", "rank2", "equal12_near", "axis_plane", "negative")
        w = worst.setdefault(fam, dict(ev=0.0, unit=0.0, res=0.0, vec=0.0, n=0, accepted=0))
        w["n"] += 1
        w["accepted"] += int(accepted)
        for k, r in (("ev", r_ev), ("unit", r_unit), ("res", r_res), ("vec", r_vec)):
            w[k] = max(w[k], r)
        if not (ev[0] <= ev[1] <= ev[2]) or max(r_ev, r_unit, r_res, r_vec) > 1 or not np.isfinite([r_ev, r_unit, r_res, r_vec]).all() or (must_accept and not accepted):
            fails.append((i, fam, ev.tolist(), lr.tolist(), dict(ev=r_ev, unit=r_unit, res=r_res, vec=r_vec, accepted=accepted, like=like)))
    print()
    for fam, w in worst.items():
        print("fx_eig3 %-14s %3d matrices, closed form accepted on %3d, worst error / bound: eigenvalues %.3g, unit %.3g, residual %.3g, vector %.3g"
              % (fam, w["n"], w["accepted"], w["ev"], w["unit"], w["res"], w["vec"]))
    assert not fails, fails[:5]
    assert worst["diagonal"]["accepted"] == 0  # (the flag does tell the two paths apart)
