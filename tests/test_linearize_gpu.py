"""The window's linearisation on the device - wc_window_linearize (k_lin_fused / k_lin_surfel / k_lin_imu, k_gather) and
wc_window_evaluate - against the short-sum reference of tests/linearize_ref.py, entry by entry in each entry's own scale:
    eH = max |H - H_ref|_ij / sqrt(H_ref_ii H_ref_jj),   eg = max |g - g_ref|_i / (sqrt(H_ref_ii) sqrt(2 c_ref))
over all entries and for each of the 4 x 4 pairs of unknown types (rot, pos, b1, b2) on its own, the cost, exact symmetry, exact
zeros where the reference has none of J (gauge rows; bias rows without IMU factors), the reference's entry sparsity at 3 x 3
sub-block granularity, and the residuals class by class (surfel residuals; each of the twelve IMU components) against the class's
own largest value.  The bars of tests/test_window_gpu.py are relative to max|H| (1e9, a bias x bias entry) and to max|g|: they
let a missing rot x b2 sub-block (entries 0.4) and bias rows of g wrong in the fifth digit through (tests/test_linearize_ref.py).

The bar is set from the reference side, per case and in the test: f = the oracle's own sequential sums against the reference in
the same metric; device bar 32 * max(f, 2.5e-15) for eH and eg, 32 * max(f_cost, eps) for the cost, 64 eps of the class's largest
value for residuals - plus, in the sub-blocks they reach, the allowances for the reference's own evaluation noise that
tests/linearize_ref.py sizes from what the oracle was measured to be off by against mpmath (A: the oracle's (1 - cos th) / th in Jr,
rot x rot and rot x pos; B: the loss weight of a surfel residual that differences two lever arms of tens of metres, pose x pose; its
share of the cost).  Every pair with a bias row or column, and g, stay at the plain bar.  A run with -s prints floor, device value
and bars per case; DESIGN.md 4.2 holds the values measured on the MI355X.

Windows above 127 sample states, C3 and C4 at full size get the same check inside tests/test_window_gpu.py, on the windows those
tests build anyway."""
import threading

import numpy as np
import pytest

import linearize_ref as lr

pytestmark = pytest.mark.gpu

SIZES = (2, 3, 4, 8, 40, 127)  # (171, 256 and 340: test_window_gpu.py::test_large_windows_linearize_match_oracle)
FAMILY_NS = (8, 40, 127)
LOG = []


@pytest.fixture(scope="module")
def ctx(gpu, oracle):
    """the suite's context; every case sets its own parameters (weak_imu's weights, quirks), the defaults go back in at the end; a run
    with -s then prints the table of measured values"""
    c = gpu
    yield c
    c.set_params(oracle.default_params())
    for where, ns, floor, e, allow, bar in LOG:  # (shown by a run with -s)
        if floor is None:
            print("%-52s %s" % (where, " ".join("%s %.1e/%.1e" % c_ for c_ in e)))
        else:
            print("%-52s floor eH %.1e eg %.1e cost %.1e | device eH %.1e eg %.1e cost %.1e | bars: bias pairs %.1e pose x pose %.1e rot x rot %.1e eg %.1e cost %.1e" % (
                where, floor["eH"], floor["eg"], floor["ec"], e["eH"], e["eg"], e["ec"], bar[0][2, 2], bar[0][1, 1], bar[0][0, 0], bar[1], bar[2]))
    rows = [r for r in LOG if r[2] is not None]
    if rows:
        print("worst device eH by type pair (rows / columns %s):" % " ".join(lr.TYPES))
        worst = np.max([r[3]["eH_types"] for r in rows], axis=0)
        for a in range(4):
            print("  %-3s " % lr.TYPES[a] + " ".join("%.1e" % v for v in worst[a]))
        print("worst device eg by type: " + " ".join("%.1e" % v for v in np.max([r[3]["eg_types"] for r in rows], axis=0)))


def _build(c, sp, sharded=False):
    w = sp["w"]
    c.set_params(sp["params"])
    keep = [c.to_device(a) if len(a) else None for a in (w["surf"], w["pose"], sp["pairs"], w["fix_surf"], w["fix_pose"], sp["pf"])]
    if not len(sp["pf"]):
        keep[3] = keep[4] = keep[5] = None
    c.window_build(keep[0], keep[1], keep[2], len(sp["pairs"]), sp["imu"], w["sample_times"], w["grav"], sp["fix_first"], keep[3], keep[4], keep[5],
                   len(sp["pf"]), sharded=sharded)
    return keep


def _device(c, ns, seed, residuals=True):
    out = []
    for x in (np.zeros(12 * ns), lr.random_point(ns, seed)):
        H, g, cost = c.window_linearize(x)
        r = dict(x=x, H=H, g=g, cost=cost)
        if residuals:
            r["eval_cost"], r["res"] = c.window_evaluate(x, want_residuals=True)
        out.append(r)
    return out


def _check(c, oracle, sp, tag, seed=1):
    keep = _build(c, sp)
    ns = len(sp["w"]["sample_times"])
    W = lr.oracle_window(oracle, sp)
    cnt = W.counts()
    nb, nu, ni, pieces = c.window_counts()
    assert (nb, nu, ni) == (cnt[0] + cnt[1] + cnt[2], cnt[3], cnt[4] + cnt[5]), tag
    lr.check_linearization(oracle, sp, _device(c, ns, seed), tag, W=W, log=LOG)
    del keep
    return cnt, pieces


@pytest.mark.parametrize("ns", SIZES)
def test_window_sizes(ctx, oracle, ns):
    """the default family (gauge held, IMU factors) across the solver's shapes: 2 and 3 sample states (one IMU factor mode only at 2),
    4 and 8, 40, and 127 - C4's count"""
    _check(ctx, oracle, lr.from_problem(lr.window_problem(oracle, ns)), "default ns=%d" % ns, seed=ns)


@pytest.mark.parametrize("family", lr.FAMILIES[1:])
@pytest.mark.parametrize("ns", FAMILY_NS)
def test_families(ctx, oracle, ns, family):
    """free_gauge (no row zeroed), no_imu (k_lin_surfel's launches per family; every bias row exactly zero), one_plane (degenerate
    geometry), weak_imu (IMU weights 1e-6: bias entries twelve decades down - the metric does not care)"""
    sp = lr.from_problem(lr.window_problem(oracle, ns, family))
    cnt, _ = _check(ctx, oracle, sp, "%s ns=%d" % (family, ns), seed=100 + ns)
    assert (cnt[4] + cnt[5] == 0) == (family == "no_imu")


@pytest.mark.parametrize("quirks", [1, 0])
def test_all_six_factor_modes_with_and_without_quirks(ctx, oracle, quirks):
    """the window of test_window_gpu.py::test_evaluate_and_linearize_match_oracle: hand-made Mode 2 pairs next to the matcher's, so
    that every factor mode is present, with the reference's quirks (overwritten Jacobian slots) and without"""
    from test_window_gpu import _mode2_pairs
    from wildcat_slam_amd import synth

    w = synth.surfel_window(3, 300, seed=11, fixed_patches=120, sample_dt=0.08)
    params = oracle.default_params()
    params.reference_quirks = quirks
    pairs = np.concatenate([oracle.match(w["surf"], w["pose"], w["surf"], w["pose"], True, params), _mode2_pairs(w, 25, np.random.default_rng(11))])
    pf = oracle.match(w["surf"], w["pose"], w["fix_surf"], w["fix_pose"], False, params)
    cnt, _ = _check(ctx, oracle, lr.spec(w, params, pairs, pf, True, w["imu"]), "six modes quirks=%d" % quirks, seed=7)
    assert all(c > 0 for c in cnt), cnt  # every factor mode present


def test_few_factors_short_gather_lists(ctx, oracle):
    """a dozen binary and four unary factors in eight sample states: every piece holds one or two records and every gather list one
    or two sources (C3 and C4, gather lists of hundreds: test_window_gpu.py)"""
    prob = lr.window_problem(oracle, 8)
    sp = lr.from_problem(prob)
    step = max(1, len(sp["pairs"]) // 12)
    sp["pairs"], sp["pf"] = sp["pairs"][::step][:12].copy(), sp["pf"][::max(1, len(sp["pf"]) // 4)][:4].copy()
    cnt, pieces = _check(ctx, oracle, sp, "few factors ns=8", seed=3)
    assert sum(cnt[:4]) == 16 and pieces <= 16 + cnt[4] + cnt[5]


@pytest.mark.parametrize("option", [None, ("lm_one_collective", 1)])
def test_two_rank_sharded_build(ctx, oracle, option):
    """two thread-ranks on one GPU (dist.ThreadComm, window_build(..., sharded=True), as test_window_gpu.py::test_sharded_solve_forms):
    every rank linearises collectively, in the default two-collective form (surfel factors' pose corners reduced and expanded into
    the rank's H next to the replicated IMU factors' sums) and with lm_one_collective (one packed all-reduce).  Both forms leave the
    full reduced H and g on every rank: bitwise equal between the ranks, and each judged like a one-rank result."""
    from wildcat_slam_amd import dist as wdist
    from wildcat_slam_amd import lib

    ns = 40
    sp = lr.from_problem(lr.window_problem(oracle, ns, seed=31))
    world = 2
    ctxs = [lib.Context(0) for _ in range(world)]
    shared = wdist.ThreadComm.shared(world)
    res, errors = [None] * world, []

    def run(r):
        try:
            c = ctxs[r]
            if option:
                c.set_dev_option(*option)
            c.set_comm(wdist.ThreadComm(shared, r, c))
            keep = _build(c, sp, sharded=True)
            want = wdist.packed_count(ns) if option else wdist.corner_count(ns)
            assert c.window_reduce_bytes() == 8 * want
            out = _device(c, ns, 9, residuals=False)
            for o in out:
                o["eval_cost"] = c.window_evaluate(o["x"])
            res[r] = (out, keep)
        except Exception as e:  # pragma: no cover
            errors.append(e)
            shared["bar"].abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    try:
        assert not errors, errors
        assert shared["calls"][0] == shared["calls"][1] > 0
        for a, b in zip(res[0][0], res[1][0]):
            assert np.array_equal(a["H"], b["H"]) and np.array_equal(a["g"], b["g"]) and a["cost"] == b["cost"] and a["eval_cost"] == b["eval_cost"], "ranks diverged"
        lr.check_linearization(oracle, sp, res[0][0], "two ranks %s" % ("one collective" if option else "two collectives"), log=LOG)
    finally:
        for c in ctxs:
            c.close()
