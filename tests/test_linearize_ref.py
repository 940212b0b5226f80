"""tests/linearize_ref.py checked on the CPU, with nothing of the library involved: the short-sum reference against itself at another
chunk length and against the oracle's sequential sums (the floor the device bar is set from); the oracle's own factor evaluation
against mpmath (the constants the allowances are multiples of); and the evidence that the scaled metric is the stronger bar - faults
planted into the oracle's own H and g that pass a copy of every bar tests/test_window_gpu.py had, and that the metric flags by orders
of magnitude with the very bars, allowances included, that a device result gets."""
import numpy as np
import pytest

import linearize_ref as lr


def _points(ns, seed=5):
    return np.zeros(12 * ns), lr.random_point(ns, seed)


def test_sum2_keeps_what_a_plain_sum_loses():
    acc = lr.Sum2(3)
    for a in (np.array([1e16, 1.0, 3.0]), np.array([1.0, 1e-17, 4.0]), np.array([-1e16, 1.0, -7.0])):
        acc.add(a)
    assert acc.value().tolist() == [1.0, 2.0, 0.0]
    acc.add(np.array([0.5]), np.array([1]))  # a subset of the entries
    assert acc.value().tolist() == [1.0, 2.5, 0.0]
    rng = np.random.default_rng(0)
    terms = rng.normal(size=(400, 50)) * 10.0 ** rng.integers(-8, 9, size=(400, 50))
    acc = lr.Sum2(50)
    for t in terms:
        acc.add(t)
    import math

    exact = np.array([math.fsum(terms[:, k]) for k in range(50)])
    assert np.all(np.abs(acc.value() - exact) <= np.spacing(np.abs(exact)))


@pytest.mark.parametrize("ns,family", [(8, "default"), (40, "default"), (40, "free_gauge"), (40, "no_imu"), (127, "default")])
def test_reference_agrees_with_itself_and_the_oracle_sits_at_the_floor(oracle, ns, family):
    """chunk-16 and chunk-64 references agree to a few 1e-16; the oracle's sequential H, g and cost are within the measured floor of the
    reference; rows without a factor (the gauge's, the bias rows of a window without IMU factors) are exactly zero on both sides"""
    sp = lr.from_problem(lr.window_problem(oracle, ns, family))
    W = lr.oracle_window(oracle, sp)
    for x in _points(ns):
        ref64 = lr.reference(oracle, sp, x, chunk=64)
        e16 = lr.scaled_errors(*lr.reference(oracle, sp, x, chunk=16), *ref64)
        floor = lr.scaled_errors(*W.linearize(x), *ref64)
        print("ns %d %s: chunk 16 vs 64 eH %.1e eg %.1e; oracle vs reference eH %.1e eg %.1e cost %.1e" % (
            ns, family, e16["eH"], e16["eg"], floor["eH"], floor["eg"], floor["ec"]))
        assert e16["eH"] <= 1e-15 and e16["eg"] <= 1e-15 and e16["ec"] <= 2 * lr.EPS, lr.describe(e16)
        assert floor["eH"] <= 4 * lr.FLOOR_MIN and floor["eg"] <= lr.FLOOR_MIN and floor["ec"] <= 4 * lr.EPS, lr.describe(floor)
        assert floor["dead_exact"] and e16["dead_exact"]
        assert floor["n_dead"] == (3 if family != "free_gauge" else 0) + (6 * ns if family == "no_imu" else 0)
        H_ref = ref64[0]
        assert np.array_equal(H_ref, H_ref.T)
        if family != "free_gauge":
            assert not H_ref[3:6].any() and not H_ref[:, 3:6].any() and not ref64[1][3:6].any()
        # the bar a device result of this case gets: from the floor, never below 32 * 2.5e-15
        assert lr.bars(floor)[0].max() == lr.BAR_FACTOR * max(floor["eH"], lr.FLOOR_MIN) <= 128 * lr.FLOOR_MIN and lr.within(floor, floor)


def test_chunk_length_keeps_full_size_windows_at_512_chunks():
    assert lr.chunk_length(3000) == 64 and lr.chunk_length(220_000) == 430 and lr.chunk_length(2_000_000) == 3907
    assert -(-2_000_000 // lr.chunk_length(2_000_000)) <= lr.MAX_CHUNKS


def test_planted_faults_pass_the_old_bars_and_fail_the_scaled_metric(oracle):
    """faults that the bars relative to max|H| and max|g| let through, planted into the oracle's H and g of the 40-state default window,
    against the bars a device result of that window gets (floor and allowances)"""
    ns = 40
    sp = lr.from_problem(lr.window_problem(oracle, ns))
    W = lr.oracle_window(oracle, sp)
    x1 = lr.random_point(ns, 5)
    for x in (np.zeros(12 * ns), x1):
        ref = lr.reference(oracle, sp, x)
        H0, g0, c0 = W.linearize(x)
        floor = lr.scaled_errors(H0, g0, c0, *ref)
        assert lr.within(floor, floor) and all(lr.old_bars(H0, g0, c0, H0, g0, c0).values())
        allow = lr.allowances(sp, x, ref[0], ref[2])
        bH, bg, _ = lr.bars(floor, allow)
        assert np.all(bH[2:, :] == lr.BAR_FACTOR * lr.FLOOR_MIN) and np.all(bH[:, 2:] == lr.BAR_FACTOR * lr.FLOOR_MIN)  # bias pairs: the plain bar
        assert bH.max() <= 2e-11 and (np.any(x) or bH[0, 0] == bH[1, 1])  # pose x pose: B, and A at the random point only
        rot_b1 = [np.abs(H0[12 * b:12 * b + 3, 12 * b + 6:12 * b + 9]).max() for b in range(ns)]
        k = 12 * int(np.argmax(rot_b1))  # the diagonal block with the largest rot x b1 entries: 4e3 next to rot x b2 entries below 1
        assert 0.1 < np.abs(H0[k:k + 3, k + 9:k + 12]).max() < 1.0 and max(rot_b1) > 1e3 and np.abs(H0[k + 9:k + 12, k + 9:k + 12]).max() > 1e8

        def planted(name, H, g, old, least):
            e = lr.scaled_errors(H, g, c0, *ref)
            passed = lr.old_bars(H, g, c0, H0, g0, c0)
            print("%-34s eH %.1e eg %.1e   old bars pass: %s" % (name, e["eH"], e["eg"], passed))
            for bar in old:
                assert passed[bar], (name, bar)
            assert not lr.within(e, floor, allow), name
            assert max((e["eH_types"] / bH).max(), e["eg"] / bg) >= least, (name, e["eH"], e["eg"])
            return e

        # the rot x b2 sub-block of one diagonal block missing: entries up to 0.42 in block k pass the bars of the full-size tests (1e-9
        # of max|H| = 1.05e9), entries up to 0.04 in the last block also the 1e-10 of the small ones
        for kk, old in ((k, ("large", "golden")), (12 * (ns - 1), ("small", "large", "golden"))):
            H = H0.copy()
            H[kk:kk + 3, kk + 9:kk + 12] = 0.0
            H[kk + 9:kk + 12, kk:kk + 3] = 0.0
            e = planted("rot x b2 sub-block zeroed, block %d" % (kk // 12), H, g0, old, 1e3)
            assert np.argmax(e["eH_types"]) in (3, 12) and ("rot x b2" in e["where_H"] or "b2 x rot" in e["where_H"])
            assert np.any(lr.subblock_nonzero(H) != lr.subblock_nonzero(H0))  # ... and the sub-block sparsity sees it, the block sparsity does not
        # the rot x b1 sub-block of one diagonal block times 1 + 1e-6
        H = H0.copy()
        H[k:k + 3, k + 6:k + 9] *= 1 + 1e-6
        H[k + 6:k + 9, k:k + 3] *= 1 + 1e-6
        e = planted("rot x b1 sub-block * (1 + 1e-6)", H, g0, ("small", "large", "golden"), 30.0)
        assert np.argmax(e["eH_types"]) in (2, 8)
        # one entry of a far 6 x 6 pose corner dropped (block pair more than two sample blocks apart): large enough for the old bars too
        far = [(a, b) for a in range(ns) for b in range(a + 3, ns) if H0[12 * a + 1, 12 * b + 4] != 0]
        a, b = far[len(far) // 2]
        H = H0.copy()
        H[12 * a + 1, 12 * b + 4] = H[12 * b + 4, 12 * a + 1] = 0.0
        planted("one entry of a far pose corner dropped", H, g0, (), 1e4)
        # every bias row of g scaled
        bias = np.nonzero(np.arange(12 * ns) % 12 >= 6)[0]
        for factor, old in ((1 + 2e-5, ("small", "large")), (1 + 2e-4, ("large",))):
            g = g0.copy()
            g[bias] *= factor
            if not np.any(x):  # (which old bar a factor passes is a matter of x = 0; at the random point the bias rows of g hold max|g|)
                e = planted("bias rows of g * (1 + %.0e)" % (factor - 1), H0, g, old, 30.0)
                assert np.argmax(e["eg_types"]) >= 2
            else:
                assert not lr.within(lr.scaled_errors(H0, g, c0, *ref), floor, allow)


def test_residual_classes_are_judged_in_their_own_scale(oracle):
    """at x = 0 the IMU residuals are 1e-3 and below next to surfel residuals of 0.4, components 6-11 exactly zero (equal biases); an
    IMU residual wrong in its seventh digit passes one bar over all residuals and fails its class; the random point reaches components 6-11"""
    ns = 40
    sp = lr.from_problem(lr.window_problem(oracle, ns))
    W = lr.oracle_window(oracle, sp)
    _, res0 = W.evaluate(np.zeros(12 * ns), want_residuals=True)
    n_surfel = len(res0) - 12 * (W.counts()[4] + W.counts()[5])
    classes = lr.residual_errors(res0, res0, n_surfel)
    assert lr.residuals_within(classes) and len(classes) == 13
    scale = dict((c[0], c[2]) for c in classes)
    assert scale["surfel"] > 0.1 and all(0 < scale["imu[%d]" % k] < 2e-3 for k in range(6)) and all(scale["imu[%d]" % k] == 0 for k in range(6, 12))
    x0 = np.zeros(12 * ns)
    H0, _, c0 = W.linearize(x0)
    allow = lr.allowances(sp, x0, H0, c0)  # (what a device result is given)
    assert allow["acc"] <= 1e-15 and allow["gyr"] <= 1e-12 and allow["surfel"] <= 4e-12
    bad = res0.copy()
    bad[n_surfel:] *= 1 + 1e-7
    assert np.abs(bad - res0).max() <= 1e-9 * np.abs(res0).max()  # the bar the suite had
    wrong = [c[0] for c in lr.residual_errors(bad, res0, n_surfel) if c[1] > lr.residual_bar(c[0], c[2], allow)]
    assert not lr.residuals_within(lr.residual_errors(bad, res0, n_surfel), allow) and set(wrong) >= {"imu[0]", "imu[2]", "imu[3]", "imu[4]", "imu[5]"}, wrong
    bad = res0.copy()
    bad[n_surfel + 7] = 1e-300  # a class that is zero in the reference is exactly zero
    assert not lr.residuals_within(lr.residual_errors(bad, res0, n_surfel))
    _, res1 = W.evaluate(lr.random_point(ns, 5), want_residuals=True)
    assert all(c[2] > 0 for c in lr.residual_errors(res1, res1, n_surfel))


def test_check_linearization_accepts_the_oracle_and_names_a_planted_fault(oracle):
    """the assertions of the device tests, run on the oracle's own results in the device's place: they pass as they are, and each of
    a lost sub-block, a written structural zero, an asymmetric entry and a scaled IMU residual is refused"""
    ns = 8
    sp = lr.from_problem(lr.window_problem(oracle, ns))
    W = lr.oracle_window(oracle, sp)

    def results():
        out = []
        for x in _points(ns):
            H, g, c = W.linearize(x)
            ec, res = W.evaluate(x, want_residuals=True)
            out.append(dict(x=x, H=H, g=g, cost=c, eval_cost=ec, res=res))
        return out

    log = []
    assert len(lr.check_linearization(oracle, sp, results(), "oracle", W=W, log=log)) == 2 and len(log) == 4
    assert all(len(entry) == 6 for entry in log)

    def lost(r):
        r["H"][12:15, 21:24] = 0.0
        r["H"][21:24, 12:15] = 0.0

    def written(r):  # pos x b1 is structurally zero
        r["H"][15, 18] = r["H"][18, 15] = 1e-30

    def asymmetric(r):
        r["H"][13, 2] = np.nextafter(r["H"][13, 2], np.inf)

    def residual(r):
        r["res"][-12:] *= 1 + 1e-6

    def gauge(r):
        r["g"][4] = 1e-300

    for point in (0, 1):
        for fault, words in ((lost, "above the bar"), (written, "sub-block"), (asymmetric, ""), (residual, "residual classes"), (gauge, "zero reference diagonal")):
            res = results()
            fault(res[point])
            with pytest.raises(AssertionError) as err:
                lr.check_linearization(oracle, sp, res, fault.__name__, W=W)
            assert words in str(err.value), (fault.__name__, str(err.value)[:300])


# ---- the oracle's own factor evaluation against mpmath: what the allowances of tests/linearize_ref.py are multiples of ---------------------
def _mp_qmul(a, b):
    return [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]]


def _mp_qrot(q, v):
    r = _mp_qmul(_mp_qmul(q, [0] + list(v)), [q[0], -q[1], -q[2], -q[3]])
    n = sum(c * c for c in q)
    return [c / n for c in r[1:]]


def test_oracle_jr_noise_is_the_constant_of_allowance_a(oracle):
    """Jr of the oracle (the (1 - cos th) / th form) against 40 digits: off by at most JR_NOISE u / th, and not by much less"""
    import mpmath as mp

    mp.mp.dps = 40
    rng = np.random.default_rng(0)
    worst = 0.0
    for th in (3e-3, 1e-3, 3e-4, 1e-4):
        for _ in range(200):
            v = rng.normal(size=3)
            v *= th / np.linalg.norm(v)
            J = np.array(oracle.so3_jr(v)).reshape(3, 3)
            m = [mp.mpf(float(a)) for a in v]
            t = mp.sqrt(sum(a * a for a in m))
            K = mp.matrix([[0, -m[2], m[1]], [m[2], 0, -m[0]], [-m[1], m[0], 0]])
            E = mp.eye(3) - ((1 - mp.cos(t)) / t ** 2) * K + ((t - mp.sin(t)) / t ** 3) * (K * K)
            err = max(abs(mp.mpf(float(J[i, j])) - E[i, j]) for i in range(3) for j in range(3))
            worst = max(worst, float(err * t) / lr.U)
    print("oracle Jr against mpmath: at most %.2f u / th" % worst)
    assert 0.2 <= worst <= lr.JR_NOISE


def test_oracle_surfel_residual_noise_is_the_constant_of_allowance_b(oracle):
    """every unary factor of the 8-state window on its own: the oracle's residual against w n . (R1 a1 + p1 - Exp(r) R2 a2 - t - p2) in
    40 digits (w n taken from the factor's own J^T r, which is products only), in units of u w S, S = |a1| + |a2| + |p1| + |p2|:
    the largest at most RES_NOISE, the root mean square at most RES_RMS, and neither much less"""
    import mpmath as mp

    mp.mp.dps = 40
    M = lambda a: [mp.mpf(float(c)) for c in a]  # noqa: E731
    ns = 8
    sp = lr.from_problem(lr.window_problem(oracle, ns))
    sp["fix_first"] = False  # (the gauge would zero the rows of g that w n is read from)
    w, b = sp["w"], sp["params"].cauchy_a ** 2
    x = lr.random_point(ns, 8)
    X, st = x.reshape(ns, 12), np.asarray(w["sample_times"])
    ratio = []
    for k in range(len(sp["pf"])):
        pf = sp["pf"][k:k + 1]
        W = lr._window(oracle, sp, None, pf, None)
        c, res = W.evaluate(x, want_residuals=True)
        rc = res[0]
        r = np.sign(rc) * np.sqrt(b * np.expm1(2 * c / b))  # the uncorrected residual, from the factor's cost 1/2 b log(1 + r^2 / b)
        _, g, _ = W.linearize(x)
        i1, i2 = int(pf["first"][0]), int(pf["second"][0])
        t = w["surf"]["t"][i2]
        l = np.searchsorted(st, t, side="right") - 1
        f = mp.mpf(float((t - st[l]) / (st[l + 1] - st[l])))
        wn = -(g[12 * l + 3:12 * l + 6] + g[12 * l + 15:12 * l + 18]) / rc * (r / rc)  # g_pos = -sqrt(rho') w n * sqrt(rho') r
        rs = [(1 - f) * a + f * c_ for a, c_ in zip(M(X[l, 0:3]), M(X[l + 1, 0:3]))]
        ts = [(1 - f) * a + f * c_ for a, c_ in zip(M(X[l, 3:6]), M(X[l + 1, 3:6]))]
        th = mp.sqrt(sum(a * a for a in rs))
        E = [mp.cos(th / 2)] + [mp.sin(th / 2) / th * a for a in rs]
        c1w = [a + p for a, p in zip(_mp_qrot(M(w["fix_pose"]["quat"][i1]), M(w["fix_surf"]["center"][i1])), M(w["fix_pose"]["pos"][i1]))]
        term2 = _mp_qrot(_mp_qmul(E, M(w["pose"]["quat"][i2])), M(w["surf"]["center"][i2]))
        d = [a - b_ - c_ - e for a, b_, c_, e in zip(c1w, term2, ts, M(w["pose"]["pos"][i2]))]
        exact = sum(mp.mpf(float(a)) * b_ for a, b_ in zip(wn, d))
        S = sum(np.linalg.norm(v) for v in (w["fix_surf"]["center"][i1], w["surf"]["center"][i2], w["fix_pose"]["pos"][i1], w["pose"]["pos"][i2]))
        ratio.append(float(abs(mp.mpf(float(r)) - exact)) / (lr.U * np.linalg.norm(wn) * S))
    ratio = np.array(ratio)
    print("oracle surfel residual against mpmath, %d factors, in u w S: max %.2f rms %.2f" % (len(ratio), ratio.max(), np.sqrt(np.mean(ratio ** 2))))
    assert len(ratio) >= 50
    assert 0.25 <= ratio.max() <= lr.RES_NOISE and 0.08 <= np.sqrt(np.mean(ratio ** 2)) <= lr.RES_RMS
