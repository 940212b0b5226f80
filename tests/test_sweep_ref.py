"""tests/sweep_ref.py - the longdouble reference tests/test_sweep_precision_gpu.py measures the sweep preparation and the pose update
against - is itself held, without a GPU: against closed forms for unit quaternions (slerp = q_a exp(f log(q_a^-1 q_b)), rotation = the
matrix form) to longdouble rounding, against the CPU oracle on every input of the GPU tests (same keep masks, fp32 outputs equal to the
cast reference up to the tie clause, fp64 outputs within the bounds), and for what the GPU tests rely on: at most TIE_CAP coordinates
of a cloud under the tie clause, every planted edge really reached."""
import numpy as np
import pytest

import sweep_ref as S
from wildcat_slam_amd import records as R
from wildcat_slam_amd import synth

LD = S.LD
E63 = 2.0**-63


def test_layouts_and_extrinsic_are_the_library_s():
    for a, b in ((S.POINT, R.POINT), (S.SURFEL, R.SURFEL), (S.POSE, R.POSE), (S.IMU_STATE, R.IMU_STATE)):
        assert a.itemsize == b.itemsize and a.names == b.names and all(a.fields[k][:2] == b.fields[k][:2] for k in a.names)
    q, t = S.ext("lidar2imu")
    assert np.abs(q - synth.mat_to_quat(synth.EXT_R[None])[0]).max() < 1e-15 and np.array_equal(t, synth.EXT_T)
    assert np.abs(S.qmat(q.astype(LD)).astype(np.float64) - synth.EXT_R).max() < 1e-7


def _unit(rng, n):
    q = rng.normal(size=(n, 4)).astype(LD)
    return q / np.sqrt((q * q).sum(-1, keepdims=True))


def test_slerp_and_rotation_against_closed_forms():
    rng = np.random.default_rng(S.SEED)
    n = 4000
    a, b = _unit(rng, n), _unit(rng, n)
    b[: n // 4] = S.qmul(a[: n // 4], S._qexp(rng.normal(size=(n // 4, 3)) * 1e-3).astype(LD))  # small angles too
    b = b / np.sqrt((b * b).sum(-1, keepdims=True))
    f = rng.uniform(0, 1, n).astype(LD)
    q, d = S.qslerp(a, f, b)
    assert (d < 0).sum() > n // 4 and (d > 0).sum() > n // 4
    # q_a exp(f log(q_a^-1 q_b')), b' = b on a's hemisphere
    bb = np.where((d < 0)[:, None], -b, b)
    r = S.qmul(S.qconj(a), bb)
    vn = np.sqrt((r[:, 1:] ** 2).sum(-1))
    half = np.arctan2(vn, r[:, 0])
    ax = r[:, 1:] / vn[:, None]
    e = np.concatenate([np.cos(f * half)[:, None], np.sin(f * half)[:, None] * ax], -1)
    closed = S.qmul(a, e)
    # acos near 1 loses half the digits of a SMALL angle, but the weights depend on it only in second order: longdouble rounding
    err = np.abs(q - closed).max().astype(np.float64)
    print("\nslerp vs closed form: %.3g (2^-63 = %.3g)" % (err, E63))
    assert err <= 16 * E63
    q0, _ = S.qslerp(a, np.zeros(n, LD), b)
    q1, _ = S.qslerp(a, np.ones(n, LD), b)
    assert np.array_equal(q0, a)
    assert np.abs(q1 - bb).max() <= 4 * E63  # sin(th) / sin(th) = 1 exactly; (1 - 1) th = 0 exactly
    v = (rng.normal(size=(n, 3)) * 50).astype(LD)
    rot = S.qrot(a, v)
    mat = np.matmul(S.qmat(a), v[..., None])[..., 0]
    assert (np.abs(rot - mat).max(axis=1) / np.sqrt((v * v).sum(-1))).max() <= 16 * E63
    # the linear branch on both sides of 1 - eps, and d exactly as built
    one = np.array([[1, 0, 0, 0]], LD)
    for e_, lin in ((2.0**-53, True), (2.0**-51, False)):
        c = 1.0 - e_
        bq = np.array([[c, np.sqrt(1.0 - c * c), 0, 0]], np.float64).astype(LD)
        qq, dd = S.qslerp(one, np.array([0.25], LD), bq)
        assert dd[0] == LD(c) and (dd[0] >= S.ONE_EPS) == lin
        assert np.abs(qq - (0.75 * one + 0.25 * bq)).max() <= 2.0**-53  # the branches differ by f (1 - f) th^2 / 2: 2^-54 at most at the threshold, 0.75 2^-53 here


def test_f32_round_knows_the_boundaries():
    w = np.array([1.0, 1.0 + 2.0**-24, 1.0 + 2.0**-24 + 2.0**-40, 1.0 - 2.0**-25, 3.0e-3], np.float64).astype(LD)
    f, dist, other = S.f32_round(w)
    assert f[0] == 1 and dist[0] == LD(2.0**-25) and other[0] == np.nextafter(np.float32(1), np.float32(0))
    assert dist[1] == 0 and {float(f[1]), float(other[1])} == {1.0, 1.0 + 2.0**-23}
    assert f[2] == np.float32(1.0 + 2.0**-23) and dist[2] == LD(2.0**-40) and other[2] == 1
    assert dist[3] == 0
    bad, ties = S.check_f32(np.array([1.0, 1.0, 1.0, 1.0, 3.0e-3], np.float32), w, 2.0**-39)
    assert ties == 3 and list(bad) == [False, False, False, False, False]
    bad, ties = S.check_f32(np.array([1.0, 1.0, 1.0, 1.0, 3.0e-3], np.float32), w, 2.0**-41)
    assert ties == 2 and list(bad) == [False, False, True, False, False]
    assert S.check_f32(np.nextafter(w.astype(np.float32), np.float32(9)), w, 2.0**-41)[0][[0, 2, 4]].all()  # (1 and 3 are ties)


def test_monotonic_restatement_is_the_sequential_loop():
    rng = np.random.default_rng(S.SEED + 1)
    for trial in range(200):
        n = int(rng.integers(1, 40))
        t = np.sort(rng.uniform(0, 1, n))
        for _ in range(int(rng.integers(0, 3))):
            t[rng.integers(0, n)] = rng.uniform(0, 1)
        keep = rng.uniform(size=n) < 0.6
        prev = [-np.inf, 0.0, 0.5][trial % 3]
        last, ok = prev, True
        for i in range(n):
            ok &= bool(t[i] >= last)
            if keep[i]:
                last = t[i]
        assert S.monotonic(t, keep, prev)[0] == ok


# ---- against the CPU oracle, on every input of the GPU tests ---------------------------------------------------------------------
@pytest.mark.parametrize("case", S.undistort_cases(), ids=lambda c: "%s-%d-%d" % c)
def test_undistort_reference_against_oracle(oracle, case):
    pts, imu = S.cloud(*case)
    ref = S.cached(("und",) + case, lambda: S.undistort(pts, imu))
    assert ref["ok"].all()
    rc, out = oracle.undistort_sweep(pts, imu)
    assert rc == 0
    got = np.stack([out["x"], out["y"], out["z"]], -1)
    bad, ties = S.check_f32(got, ref["w"], ref["bound"][:, None])
    assert ties <= S.TIE_CAP, "choose another seed"
    assert not bad.any()
    raw_in, raw_out = pts.view(np.uint8).reshape(-1, 48), out.view(np.uint8).reshape(-1, 48)
    assert np.array_equal(raw_in[:, 12:], raw_out[:, 12:])
    # what the case is there for
    size, n = len(imu), len(pts)
    on_state = np.isin(pts["time"], imu["t"])
    assert (ref["fac"][on_state] == 1).all() and (ref["fac"] > 0).all() and (ref["fac"] <= 1).all()
    assert np.array_equal(imu["t"][ref["lo"][on_state]], pts["time"][on_state])
    assert (pts["time"] == imu["t"][-1]).any()
    if n >= 1000 and size > 2:
        assert on_state.sum() >= 31
        for name, i in S.PLANT.items():
            assert (ref["lo"] == i + 1).sum() >= 3, name
        d = ref["d"]
        assert (d[ref["lo"] == S.PLANT["lin"] + 1] == LD(1.0 - 2.0**-53)).all() and (d[ref["lo"] == S.PLANT["slerp"] + 1] == LD(1.0 - 2.0**-51)).all()
        assert (np.abs(np.abs(d[ref["lo"] == S.PLANT["half"] + 1]) - 1e-3) < 1e-4).all()
        if case[0] == "signs":
            assert (d < 0).sum() > n // 4
    assert np.abs(ref["d"]).min() > 5e-4  # no interval near the discontinuity of the sign flip


def test_undistort_range_errors_in_the_reference(oracle):
    pts, imu = S.cloud("smooth", 37, 257)
    for idx, t in ((0, imu["t"][0]), (256, imu["t"][0]), (100, np.nextafter(imu["t"][-1], np.inf))):
        p = pts.copy()
        p["time"][idx] = t
        assert not S.undistort(p, imu)["ok"][idx] and oracle.undistort_sweep(p, imu)[0] == 2


@pytest.mark.parametrize("case", S.pose_cases(), ids=lambda c: "%s-%d-%d" % c)
def test_pose_reference_against_oracle(oracle, case):
    surf, flags, imu = S.surfels(*case)
    n = len(surf)
    if n > 1:
        assert min((flags == 0).sum(), (flags == 1).sum()) * 3 >= n
    ref = S.cached(("pose",) + case, lambda: S.update_poses(imu, surf, flags))
    assert ref["ok"].all()
    s, pose, fl = surf.copy(), np.zeros(n, R.POSE), flags.copy()
    assert oracle.update_surfel_poses(imu, s, pose, fl) == 0
    ratios = S.compare_poses(ref, surf, flags, s, pose, fl)
    print("\n%s: " % (case,) + ", ".join("%s %.3g" % kv for kv in ratios.items()))
    for k, v in ratios.items():
        assert v <= 1.0, (k, v)


@pytest.mark.parametrize("name", list(S.prefilter_cases()))
def test_prefilter_reference_against_oracle(oracle, name):
    pts, args = S.prefilter_cases()[name]()
    ref = S.cached(("pre", name), lambda: S.prefilter(pts, *args))
    out = oracle.prefilter_points(pts, *args)
    ties = int((ref["dist"].astype(np.float64) <= ref["bound"][:, None]).sum())
    assert ties <= S.TIE_CAP, "choose another seed"
    assert len(out) == ref["keep"].sum() and np.array_equal(out["time"], ref["out"]["time"])  # stamps are unique: same mask, same order
    S.compare_survivors(out, ref, padding=False)  # (pyoracle returns a numpy copy)
    kept = int(ref["keep"].sum())
    n = len(pts)
    if name.startswith("none"):
        assert kept == 0
    elif name.startswith("all"):
        assert kept == n
    elif name.startswith("alternate"):
        assert np.array_equal(ref["keep"], np.arange(n) % 2 == 0)
    elif name.startswith("runs"):
        assert np.array_equal(ref["keep"], (np.arange(n) // S.RUN) % 2 == 0) and S.RUN > 8192
    elif name.startswith("random") and n >= 255:
        assert 0.2 * n < kept < 0.8 * n and ref["blind"].sum() > 0.05 * n


@pytest.mark.parametrize("e", S.EXTS)
def test_planted_edges_are_reached(e):
    pts, args, G = S.range_edges(e)
    ref = S.prefilter(pts, *args)
    assert not ref["blind"].any()
    for lim in (S.MIN_RANGE, S.MAX_RANGE):
        l32 = np.float32(lim)
        dn, up = np.nextafter(l32, np.float32(0)), np.nextafter(l32, np.float32(1e9))
        nrm, keep = ref["nrm"][G["axis%g" % lim]], ref["keep"][G["axis%g" % lim]]
        for v in (dn, l32, up):
            assert (nrm == v).sum() >= (6 if e == "identity" else 1), (lim, v)  # (with the offset not every axis reaches every value)
        if lim == S.MIN_RANGE:  # float32(0.3) > 0.3
            assert keep[nrm == l32].all() and not keep[nrm == dn].any()
        else:  # 120 is a float
            assert keep[nrm == l32].all() and not keep[nrm == up].any()
        for key in ("fused", "dbl"):
            idx = G["%s%g" % (key, lim)]
            assert len(idx) >= 4, (key, lim)
            plain, fused, dbl = S.norm_variants(ref["xyz"][idx])
            assert np.array_equal(S._in_range(plain), ref["keep"][idx])
            assert (S._in_range(plain) != S._in_range(fused if key == "fused" else dbl)).all()
    pts, args, G = S.blind_edges(e)
    ref = S.prefilter(pts, *args)
    hit = 0
    for a in range(3):
        for side in (0, 1):
            idx = G[(a, side)]
            face = np.float32(S.BOX_EXACT[side][a])
            outside = np.nextafter(face, np.float32(-9 if side == 0 else 9))
            inside = np.nextafter(face, np.float32(0))
            c, keep = ref["xyz"][idx, a], ref["keep"][idx]
            # with the lidar -> imu offset no fp32 input maps onto some faces (-in + t rounds past them): the nearest floats either side
            # are reached on every face, the face itself wherever the identity is used and on `hit` faces otherwise
            assert (c == outside).any() and ((c == face).any() or (c == inside).any())
            hit += int((c == face).any())
            assert not keep[c == face].any() and not keep[c == inside].any() and keep[c == outside].all()  # inclusive faces
            assert np.array_equal(keep, ~ref["blind"][idx])  # the box alone decides: the norm is in range
    print("\n%s: faces hit exactly %d of 6" % (e, hit))
    assert hit >= (6 if e == "identity" else 3)
    assert ref["keep"][G["nan"]].all() and np.isnan(ref["xyz"][G["nan"]]).all()  # every comparison with a NaN is false: kept


def test_reverse_copy_reference():
    s, p = np.zeros(5, S.SURFEL), np.zeros(5, S.POSE)
    s["t"], p["pos"][:, 0] = np.arange(5), np.arange(5)
    rs, rp = S.reverse_copy(s, p)
    assert list(rs["t"]) == [4, 3, 2, 1, 0] and list(rp["pos"][:, 0]) == [4, 3, 2, 1, 0]
