"""The per-point and per-surfel stages in front of the hot path - k_prefilter_flags / _scatter / _monotonic and k_undistort<PACKED>
(csrc/sweep.hip), k_update_poses and k_reverse_copy (csrc/poses.hip) - against tests/sweep_ref.py, a numpy longdouble restatement of
what the reference program computes, per point and per surfel, each in its OWN scale: no scale of a whole cloud or a whole field.
U = 2^-53.  All constants come from operation counts and input magnitudes, none from what a kernel returned:

  undistorted coordinate  the kernel's float must EQUAL float32(w), w the reference's longdouble value.  Only where w lies within
                          B_w = 16 U (|p|_2 + max|pos|) of an fp32 rounding boundary the float on the other side of that boundary is
                          allowed too (the tie clause).  B_w: ~10 rounded fp64 operations of the rotation on terms <= |p|, the slerp
                          weights to a few ulp (acos and sin of the device may differ from the host's by an ulp or two), the lerp and
                          the final addition on pos.  At most TIE_CAP = 2 coordinates of a cloud may fall under the clause: decided
                          from the reference alone and asserted in tests/test_sweep_ref.py too - a seed that gives more is replaced.
  record form             the 36 bytes of a record that are not x, y, z pass through; the packed form's time_out is the input stamp and
                          its floats are the record form's, bit for bit
  pre-filtered coordinate the same clause with B_e = 16 U (|p|_2 + |t|_inf) (the same rotation, one addition of t); with the identity
                          extrinsic every operation is exact and B_e = 0.  Keep mask, order, count and kept_times are the reference's
                          (its decisions are fp32 by definition: x*x + y*y + z*z in that order, correctly rounded sqrt, comparisons in
                          double, inclusive blind box), h_monotonic the restated CHECK's - which knows nothing of `cap`
  pose                    |d pos_k| <= 4 U max(|a.pos_k|, |b.pos_k|)   (1 - f, two products, one sum, and f's own rounding on b - a)
                          |d quat_k| <= 8 U                            (weights to ~4.5 ulp on components <= 1, two products, one sum)
  body-frame centre       |d c_k| <= 16 U (|c - pos|_2 + |pos|_inf);   normal  |d n_k| <= 16 U
  body-frame covariance   |d Cb_ij| <= 549 U |C|max: (R^T C) R with R = qmat(rot), first order.  rot carries eps_q = 8 U per component
                          (the bound above).  An entry of R is 1 or 0 plus two terms 2 q_a q_b: perturbed by <= 4 sqrt(2) eps_q < 6 eps_q
                          on the diagonal, <= 2 eps_q (|w| + |x| + |y| + |z|) <= 4 eps_q off it, plus 3 roundings of its own:
                          eps_R = 51 U.  R^T C: three products, two sums per entry: |dM| <= 3 eps_R |C|max + 3 sqrt(3) U |C|max
                          (a column of |R| sums to <= sqrt 3).  M R the same on |M| <= sqrt(3) |C|max:
                          |dCb| <= sqrt(3) |dM| + 3 sqrt(3) eps_R |C|max + 9 U |C|max = (6 sqrt(3) 51 + 18) U |C|max < 549 U |C|max.
                          Nearly all of it is the quaternion's worst case carried through; the roundings of the products alone are 18 U
  flags                   surfels whose flag was 1 keep centre, normal and covariance byte for byte and get the new pose only; every flag
                          is 1 afterwards; t, sigma, resolution untouched
  range errors            a stamp on the first state's (lower_bound gives index 0) or beyond the last state: code 2, once; a valid call on
                          the same context afterwards gives the reference's result (the status word is cleared)
  capacity                cap below the number kept: WC_ERR_CAPACITY, *h_n_out = kept, the first cap records and stamps right, the bytes
                          behind cap in both outputs untouched, h_monotonic still the restated CHECK's
  reverse copy            every byte of both arrays

Every test prints its worst error / bound ratio per field and the number of tie-clause coordinates (pytest -s); DESIGN.md section 4.4
keeps the figures."""
import numpy as np
import pytest

import sweep_ref as S
from wildcat_slam_amd import lib
from wildcat_slam_amd import records as R

pytestmark = pytest.mark.gpu
LD = S.LD
_id3 = lambda c: "%s-%d-%d" % c  # noqa: E731


def _und_ref(case):
    pts, imu = S.cloud(*case)
    return pts, imu, S.cached(("und",) + case, lambda: S.undistort(pts, imu))


def _check_undistorted(label, pts, ref, rec, xyz, t):
    got = np.stack([rec["x"], rec["y"], rec["z"]], -1)
    bad, ties = S.check_f32(got, ref["w"], ref["bound"][:, None])
    # for the record: the error in units of B_w (a float cannot show less than its own rounding: only meaningful as "far below 2^29")
    err = (np.abs(got.astype(LD) - ref["w"]).astype(np.float64) / ref["bound"][:, None]).max()
    differ = int((got != S.f32_round(ref["w"])[0]).sum())
    print("\n%s: %d coordinates, %d under the tie clause, %d not the cast reference, %d wrong; |float - w| / B_w <= %.3g" % (label, got.size, ties, differ, int(bad.sum()), err))
    assert ties <= S.TIE_CAP
    assert not bad.any(), np.flatnonzero(bad.any(axis=1))[:10]
    raw_in, raw_out = pts.view(np.uint8).reshape(-1, 48), rec.view(np.uint8).reshape(-1, 48)
    assert np.array_equal(raw_in[:, 12:], raw_out[:, 12:])
    assert t.tobytes() == np.ascontiguousarray(pts["time"]).tobytes()
    assert xyz.tobytes() == np.ascontiguousarray(got).tobytes()


@pytest.mark.parametrize("case", S.undistort_cases(), ids=_id3)
def test_undistort_record_and_packed_forms(gpu, case):
    pts, imu, ref = _und_ref(case)
    rec = gpu.undistort_sweep(pts, imu)
    xyz, t = gpu.undistort_sweep_packed(pts, imu)
    _check_undistorted(_id3(case), pts, ref, rec, xyz, t)


def _range_error_clouds():
    """(label, points, imu, index of the offending stamp)"""
    pts, imu = S.cloud("smooth", 37, 257)  # 257: a last block of one point
    first, beyond = imu["t"][0], np.nextafter(imu["t"][-1], np.inf)
    out = []
    for label, n, idx, stamp in (("first@0", 257, 0, first), ("first@n-1", 257, 256, first), ("first-alone", 1, 0, first), ("beyond", 257, 100, beyond)):
        p = pts[:n].copy()
        p["time"][idx] = stamp
        out.append((label, p, imu, idx))
    return out


@pytest.mark.parametrize("which", range(4), ids=lambda i: _range_error_clouds()[i][0])
def test_undistort_range_error_then_a_valid_call(gpu, which):
    label, p, imu, idx = _range_error_clouds()[which]
    assert not S.undistort(p, imu)["ok"][idx]
    form = gpu.undistort_sweep if which % 2 == 0 else gpu.undistort_sweep_packed
    with pytest.raises(lib.WildcatError) as e:  # once
        form(p, imu)
    assert e.value.code == 2
    case = ("smooth", 37, 257)
    pts, imu, ref = _und_ref(case)
    _check_undistorted(label + " then valid", pts, ref, gpu.undistort_sweep(pts, imu), *gpu.undistort_sweep_packed(pts, imu))


# ---- pose update -----------------------------------------------------------------------------------------------------------------
def _update(gpu, imu, surf, flags):
    n = len(surf)
    d_imu, d_s, d_p, d_b = gpu.to_device(imu), gpu.to_device(surf), gpu.alloc(56 * max(n, 1) + 64), gpu.to_device(flags)
    d_p.upload(np.full(56 * max(n, 1) + 64, 0xA5, np.uint8))
    gpu.update_surfel_poses(d_imu, len(imu), d_s, d_p, d_b, n)
    tail = d_p.download(np.uint8, 56 * n + 64)[56 * n:]
    assert (tail == 0xA5).all()
    return d_s.download(R.SURFEL, n), d_p.download(R.POSE, n), d_b.download(np.uint8, n)


@pytest.mark.parametrize("case", S.pose_cases(), ids=_id3)
def test_pose_update(gpu, case):
    surf, flags, imu = S.surfels(*case)
    n = len(surf)
    if n > 1:
        assert min((flags == 0).sum(), (flags == 1).sum()) * 3 >= n
    ref = S.cached(("pose",) + case, lambda: S.update_poses(imu, surf, flags))
    s, pose, fl = _update(gpu, imu, surf, flags)
    ratios = S.compare_poses(ref, surf, flags, s, pose, fl)
    print("\n%s: worst error / bound: " % _id3(case) + ", ".join("%s %.3g" % kv for kv in ratios.items()))
    for k, v in ratios.items():
        assert v <= 1.0, (k, v)


def test_pose_update_range_error_then_a_valid_call(gpu):
    case = ("smooth", 37, 257)
    surf, flags, imu = S.surfels(*case)
    for idx, stamp in ((0, imu["t"][0]), (256, imu["t"][0]), (100, np.nextafter(imu["t"][-1], np.inf))):
        s = surf.copy()
        s["t"][idx] = stamp
        with pytest.raises(lib.WildcatError) as e:
            _update(gpu, imu, s, flags)
        assert e.value.code == 2
        ref = S.cached(("pose",) + case, lambda: S.update_poses(imu, surf, flags))
        for k, v in S.compare_poses(ref, surf, flags, *_update(gpu, imu, surf, flags)).items():
            assert v <= 1.0, (k, v)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1000])
def test_reverse_copy_every_byte(gpu, n):
    rng = np.random.default_rng([S.SEED, 31, n])
    src_s, src_p = rng.integers(0, 256, 144 * n, dtype=np.uint8), rng.integers(0, 256, 56 * n, dtype=np.uint8)
    d_ss, d_sp = gpu.alloc(144 * n + 64), gpu.alloc(56 * n + 64)
    d_ds, d_dp = gpu.alloc(144 * n + 64), gpu.alloc(56 * n + 64)
    for d, src, size in ((d_ss, src_s, 144), (d_sp, src_p, 56), (d_ds, None, 144), (d_dp, None, 56)):
        d.upload(np.concatenate([src if src is not None else np.full(size * n, 0x3C, np.uint8), np.full(64, 0xA5, np.uint8)]))
    gpu.reverse_copy_surfels(d_ss, d_sp, n, d_ds, d_dp)
    gpu.sync()
    want_s, want_p = S.reverse_copy(src_s.view(R.SURFEL), src_p.view(R.POSE))
    got_s, got_p = d_ds.download(np.uint8, 144 * n + 64), d_dp.download(np.uint8, 56 * n + 64)
    assert got_s[: 144 * n].tobytes() == want_s.tobytes() and got_p[: 56 * n].tobytes() == want_p.tobytes()
    assert (got_s[144 * n:] == 0xA5).all() and (got_p[56 * n:] == 0xA5).all()
    assert d_ss.download(np.uint8, 144 * n).tobytes() == src_s.tobytes() and d_sp.download(np.uint8, 56 * n).tobytes() == src_p.tobytes()


# ---- pre-filter ------------------------------------------------------------------------------------------------------------------
def _pre_ref(name):
    pts, args = S.prefilter_cases()[name]()
    return pts, args, S.cached(("pre", name), lambda: S.prefilter(pts, *args))


@pytest.mark.parametrize("name", list(S.prefilter_cases()))
def test_prefilter_mask_order_coordinates_and_stamps(gpu, name):
    pts, args, ref = _pre_ref(name)
    ties = int((ref["dist"].astype(np.float64) <= ref["bound"][:, None]).sum())
    assert ties <= S.TIE_CAP
    kept = int(ref["keep"].sum())
    out, times, mono = gpu.prefilter_points_checked(pts, *args)
    assert len(out) == kept and np.array_equal(out["time"], ref["out"]["time"])  # unique stamps: the same mask in the same order
    S.compare_survivors(out, ref)
    assert times.tobytes() == np.ascontiguousarray(ref["out"]["time"]).tobytes()
    assert mono == S.monotonic(pts["time"], ref["keep"], -np.inf)[0] and mono
    plain = gpu.prefilter_points(pts, *args)
    assert plain.tobytes() == out.tobytes()
    nan = int(np.isnan(ref["xyz"]).any(axis=1).sum())
    print("\n%s: %d of %d kept, %d NaN points kept, %d coordinates under the tie clause" % (name, kept, len(pts), nan, ties))


def _raw(gpu, pts, args, cap, prev_time, want_times):
    """the call on buffers with canary bytes behind `cap` -> (rc, n_out, mono, the records' bytes + canary, the stamps' bytes + canary)"""
    d_in = gpu.to_device(pts)
    d_out, d_t = gpu.alloc(48 * cap + 64), gpu.alloc(8 * cap + 64)
    d_out.upload(np.full(48 * cap + 64, 0xA5, np.uint8))
    d_t.upload(np.full(8 * cap + 64, 0xA5, np.uint8))
    rc, m, mono = gpu.prefilter_device(d_in, len(pts), *args, d_out, cap, prev_time, d_t if want_times else None)
    return rc, m, mono, d_out.download(np.uint8, 48 * cap + 64), d_t.download(np.uint8, 8 * cap + 64)


@pytest.mark.parametrize("want_times", [True, False], ids=["kept_times", "no_kept_times"])
@pytest.mark.parametrize("violation", [False, True], ids=["monotonic", "violation_beyond_cap"])
def test_prefilter_capacity(gpu, violation, want_times):
    pts, args, _ = _pre_ref("random1000-lidar2imu")
    pts = pts.copy()
    if violation:  # the last two kept points swap stamps: the only violation lies beyond every cap below `kept`
        k = np.flatnonzero(S.prefilter(pts, *args)["keep"])[-2:]
        pts["time"][k] = pts["time"][k[::-1]]
    ref = S.prefilter(pts, *args)
    kept = int(ref["keep"].sum())
    assert 200 < kept < 800
    want_mono, bad = S.monotonic(pts["time"], ref["keep"], -np.inf)
    assert want_mono == (not violation)
    want_rec = ref["out"].view(np.uint8).reshape(-1, 48)
    want_t = np.ascontiguousarray(ref["out"]["time"]).view(np.uint8)
    for cap in (0, 1, kept - 1, kept, kept + 1):
        rc, m, mono, rec, t = _raw(gpu, pts, args, cap, -np.inf, want_times)
        assert rc == (lib.WC_ERR_CAPACITY if cap < kept else lib.WC_OK), cap
        assert m == kept and mono == want_mono, (cap, m, mono)
        k = min(cap, kept)
        got = rec[: 48 * k].reshape(-1, 48)
        assert np.array_equal(got[:, 12:], want_rec[:k, 12:])
        bad_xyz, _ = S.check_f32(np.ascontiguousarray(got[:, :12]).view(np.float32).reshape(-1, 3), ref["p"][ref["keep"]][:k], ref["bound"][ref["keep"]][:k, None])
        assert not bad_xyz.any()
        assert (rec[48 * k:] == 0xA5).all(), "records written behind cap"
        if want_times:
            assert t[: 8 * k].tobytes() == want_t[: 8 * k].tobytes() and (t[8 * k:] == 0xA5).all(), "stamps written behind cap"
        else:
            assert (t == 0xA5).all()
    # the plain entry point and the binding's cap
    rc, m, mono, rec, _ = _raw(gpu, pts, args, 1, None, False)
    assert (rc, m, mono) == (lib.WC_ERR_CAPACITY, kept, None) and (rec[48:] == 0xA5).all()
    with pytest.raises(lib.WildcatError) as e:
        gpu.prefilter_points(pts, *args, cap=kept - 1)
    assert e.value.code == lib.WC_ERR_CAPACITY
    assert len(gpu.prefilter_points(pts, *args, cap=kept)) == kept


def test_prefilter_monotonic_check(gpu):
    pts, args, ref = _pre_ref("random1000-identity")
    keep = ref["keep"]
    kept_idx = np.flatnonzero(keep)

    def run(p, prev=-np.inf, kept_times=True):
        want = S.monotonic(p["time"], keep, prev)[0]
        out, times, mono = gpu.prefilter_points_checked(p, *args, prev_time=prev, kept_times=kept_times)
        assert mono == want and (times is None) == (not kept_times) and len(out) == len(kept_idx)
        return mono

    t0 = float(pts["time"][0])
    assert run(pts) and run(pts, kept_times=False) and run(pts, prev=-np.inf)
    # point 0 against prev_time: equal passes, later fails - whether point 0 is kept or not
    assert run(pts, prev=t0) and not run(pts, prev=np.nextafter(t0, np.inf)) and not run(pts, prev=np.nextafter(t0, np.inf), kept_times=False)
    # a kept point at the end of a 256-block newer than the first point of the next block
    a = kept_idx[kept_idx % 256 == 255]
    assert len(a)
    i = int(a[0])
    p = pts.copy()
    p["time"][i] = p["time"][i + 1] + 1e-7
    assert not run(p) and not run(p, kept_times=False)
    # the same stamp on a DROPPED point does not move the reference: no violation
    dr = np.flatnonzero(~keep)
    dr = dr[(dr % 256 == 255) & (dr + 1 < len(pts))]
    assert len(dr)
    p = pts.copy()
    p["time"][int(dr[0])] = p["time"][int(dr[0]) + 1] + 1e-7
    assert run(p) and run(p, kept_times=False)
