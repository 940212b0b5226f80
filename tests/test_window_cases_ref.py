"""Every planted window of tests/window_cases.py is live on the CPU: the oracle (oracle/window.cc, the restatement of
BuildSldWinLidarResiduals / BuildFixWinLidarResiduals / BuildImuResiduals, lidar_odometry.cc:254-363, and of the CHECKs inside the
factors, cost_functor.h:367, :390) builds each accepted case to the planted kind counts, the planted sample intervals and
interpolation fractions (== 0.0 where the case says so; against exact rational arithmetic everywhere), the planted IMU triples, and
the structure of H that plain loops over the stated intervals predict; it refuses each refusal case with the planted code; and
moving the planted stamp one ulp across its edge changes the return code, a count or the structure.  The piece count a case
expects is restated here from the oracle's own factors with sorted / collections.Counter / ceil - nothing of the library."""
import collections
import fractions
import math

import numpy as np
import pytest

import linearize_ref as lr
import window_cases as wc


def _build(oracle, case):
    """(return code, oracle.Window): the reference's insertion order; the first refusal ends the construction"""
    sp = case["sp"]
    w = sp["w"]
    W = oracle.Window(w["sample_times"], w["grav"], sp["fix_first"], sp["params"])
    rc = 0
    if len(sp["pairs"]):
        rc = W.add_binary(w["surf"], w["pose"], sp["pairs"], check=False)
    if rc == 0 and len(sp["pf"]):
        rc = W.add_unary(w["fix_surf"], w["fix_pose"], w["surf"], w["pose"], sp["pf"], check=False)
    if rc == 0 and sp["imu"] is not None:
        rc = W.add_imu(sp["imu"], check=False)
    return rc, W


def _structure(W, seed=5):
    H, _, _ = W.linearize(lr.random_point(W.ns, seed))
    return lr.subblock_nonzero(H)


def _pieces(W):
    """the piece count restated from the oracle's own factors: sum over surfel keys of ceil(count / 256) + sum over runs of IMU
    factors with one first sample state of ceil(run / 8)"""
    c = W.counts()
    keys = collections.Counter((kind == 3, s1, s2) for kind, s1, s2, _, _ in (W.lidar_factor(k) for k in range(sum(c[:4]))))
    total = sum(math.ceil(n / wc.PIECE) for _, n in sorted(keys.items()))
    sp1 = [W.imu_factor(j)[1] for j in range(c[4] + c[5])]
    i = 0
    while i < len(sp1):
        j = i
        while j < len(sp1) and sp1[j] == sp1[i]:
            j += 1
        total += math.ceil((j - i) / wc.IMU_MAX)
        i = j
    return total


def _signature(oracle, case):
    """what a build decides: the return code, or the kind counts, the piece count, the IMU factors per interval and the structure of H"""
    rc, W = _build(oracle, case)
    if rc:
        return (rc,)
    per_interval = collections.Counter(W.imu_factor(j)[1] for j in range(W.counts()[4] + W.counts()[5]))  # IMU factors by first sample state
    return (0, tuple(W.counts()), _pieces(W), tuple(sorted(per_interval.items())), _structure(W).tobytes())


@pytest.mark.parametrize("name", wc.names(lambda c: c["rc"] == 0))
def test_accepted_case_is_what_it_plants(oracle, name):
    case = wc.by_name(oracle.default_params(), name)
    rc, W = _build(oracle, case)
    assert rc == 0, case["desc"]
    assert W.counts() == case["counts"], case["desc"]
    nb, nu, ni, pieces = case["shape"]
    c = case["counts"]
    assert (nb, nu, ni) == (c[0] + c[1] + c[2], c[3], c[4] + c[5])
    T = case["sp"]["w"]["sample_times"]
    # every surfel factor: the planted kind, intervals and fractions
    k = 0
    for li, (kind, s1, s2, f1, f2, count) in enumerate(case["lidar"]):
        for _ in range(count):
            got = W.lidar_factor(k)
            assert got == (kind, s1, s2, f1, f2), (case["desc"], k, got, (kind, s1, s2, f1, f2))
            k += 1
        for which, f in ((0, f1), (1, f2)):
            assert 0.0 <= f < 1.0, (case["desc"], li, which, f)
    assert k == nb + nu
    for li, which in case["f_zero"]:
        assert case["lidar"][li][3 + which] == 0.0 and W.lidar_factor(sum(l[5] for l in case["lidar"][:li]))[3 + which] == 0.0, case["desc"]
    # the fractions against exact rational arithmetic on the planted stamps: f uses the true interval (half an ulp of the
    # difference and half an ulp of the quotient: 2 eps relative, with room)
    surf = case["sp"]["w"]["surf"]
    pos = 0
    for kind, s1, s2, f1, f2, count in case["lidar"]:
        pr = (case["sp"]["pf"][pos - nb] if kind == 3 else case["sp"]["pairs"][pos])
        for seg, f, t in ((s1, f1, None if kind == 3 else surf["t"][pr["first"]]), (s2, f2, surf["t"][pr["second"]])):
            if t is None:
                continue
            num = fractions.Fraction(float(t)) - fractions.Fraction(float(T[seg]))
            den = fractions.Fraction(float(T[seg + 1])) - fractions.Fraction(float(T[seg]))
            assert abs(fractions.Fraction(f) - num / den) <= 4 * lr.EPS * (num / den), (case["desc"], seg, f, float(num / den))
        pos += count
    # every IMU factor: the planted triple
    for j, want in enumerate(case["imu_sel"]):
        assert W.imu_factor(j) == want, (case["desc"], j, W.imu_factor(j), want)
    # pieces, restated from the oracle's factors
    assert _pieces(W) == pieces, (case["desc"], _pieces(W), pieces)
    # the structure of H
    if nb + nu + ni:
        want, got = wc.expected_sparsity(case), _structure(W)
        diff = np.argwhere(want != got)
        assert len(diff) == 0, (case["desc"], "expected / oracle", [(int(a), lr.TYPES[b], int(c_), lr.TYPES[d], bool(want[a, b, c_, d])) for a, b, c_, d in diff[:8]])
    else:
        H, g, cost = W.linearize(lr.random_point(W.ns, 5))
        assert not H.any() and not g.any() and cost == 0.0


@pytest.mark.parametrize("name", wc.names(lambda c: c["rc"] != 0))
def test_refused_case_returns_the_planted_code(oracle, name):
    case = wc.by_name(oracle.default_params(), name)
    rc, _ = _build(oracle, case)
    assert rc == case["rc"], (case["desc"], rc)


@pytest.mark.parametrize("name", wc.names(lambda c: c["across"] is not None))
def test_one_ulp_across_the_edge_changes_the_build(oracle, name):
    case = wc.by_name(oracle.default_params(), name)
    here, there = _signature(oracle, case), _signature(oracle, case["across"])
    assert here[0] == case["rc"] and there[0] == case["across"]["rc"], (case["desc"], here[0], there[0])
    assert here != there, (case["desc"], "the planted stamp and its neighbour build the same problem")


def test_far_pair_is_a_pose_corner(oracle):
    """sp2l = sp1l + 2 against sp1l + 3: block pair (sp1l, sp2l + 1) goes from two to three sample blocks apart - the pair the device's
    gather treats as far (its 6 x 6 pose corner only)"""
    P = oracle.default_params()
    for d, apart in ((2, 2), (3, 3)):
        case = wc.by_name(P, "kind-plus%d" % d)
        _, s1, s2, _, _, _ = case["lidar"][0]
        assert (s2 + 1) - s1 == apart + 1 and s2 - s1 == apart
        nz = wc.expected_sparsity(case)
        assert nz[s1, :2, s2 + 1, :2].all() and not nz[s1, 2:, s2 + 1, :].any() and not nz[s1, :, s2 + 1, 2:].any()


def test_sort_width_cases_grow_a_bit(oracle):
    """the key count ns^2 + ns + 1 of each pair of sizes lies on both sides of a power of two, and the cases hold the largest key
    of both families and key ns^2"""
    P = oracle.default_params()
    for lo, hi, bits in ((90, 91, (13, 14)), (127, 128, (14, 15)), (255, 256, (16, 17))):
        assert ((lo * lo + lo).bit_length(), (hi * hi + hi).bit_length()) == bits
        for ns in (lo, hi):
            case = wc.by_name(P, "width-%d" % ns)
            keys = [(s1 * ns + s2) if kind != 3 else ns * ns + s2 for kind, s1, s2, _, _, _ in case["lidar"]]
            assert (ns - 2) * ns + ns - 2 in keys and ns * ns in keys and ns * ns + ns - 2 in keys and 0 in keys
            assert sum(case["shape"][:3]) < 64


def test_permutation_keeps_every_key_in_order(oracle):
    sp, sp_p, pb, pu = wc.permutation_pair(oracle.default_params())
    T, t = sp["w"]["sample_times"], sp["w"]["surf"]["t"]
    seg = lambda x: np.searchsorted(T, x, side="right") - 1
    for a, b, perm, key in ((sp["pairs"], sp_p["pairs"], pb, lambda p: seg(t[p["first"]]) * 100 + seg(t[p["second"]])), (sp["pf"], sp_p["pf"], pu, lambda p: seg(t[p["second"]]))):
        assert sorted(perm.tolist()) == list(range(len(a))) and np.array_equal(b, a[perm])
        ka = key(a)
        for k in np.unique(ka):
            assert np.all(np.diff(perm[key(b) == k]) > 0)  # the key's records in their old order
    assert 1800 <= len(pb) + len(pu) <= 2200
    Wa, Wb = lr.oracle_window(oracle, sp), lr.oracle_window(oracle, sp_p)
    assert Wa.counts() == Wb.counts()
    x = lr.random_point(len(T), 2)
    _, ra = Wa.evaluate(x, want_residuals=True)
    _, rb = Wb.evaluate(x, want_residuals=True)
    nb = len(pb)
    assert np.array_equal(rb[:nb], ra[:nb][pb]) and np.array_equal(rb[nb:nb + len(pu)], ra[nb:nb + len(pu)][pu]) and np.array_equal(rb[nb + len(pu):], ra[nb + len(pu):])


def test_sharded_cases(oracle):
    """three ranks: with two binary pairs and one unary pair rank 0's contiguous shares are empty; with three binary pairs the defect
    sits in the pair that only rank 1 owns"""
    P = oracle.default_params()
    share = lambda n, r, w: ((n * r) // w, (n * (r + 1)) // w - (n * r) // w)
    assert share(2, 0, 3)[1] == 0 and share(1, 0, 3)[1] == 0
    assert [share(3, r, 3) for r in range(3)] == [(0, 1), (1, 1), (2, 1)]
    for n in (2, 3, 4):
        case = wc.sharded(P, n)
        rc, W = _build(oracle, case)
        assert rc == 0 and W.counts() == case["counts"]
    bad = wc.sharded(P, 3, defect_at=1)
    assert _build(oracle, bad)[0] == wc.RANGE
