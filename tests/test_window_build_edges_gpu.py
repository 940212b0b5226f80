"""wc_window_build at its edges (csrc/window.hip: k_pair_keys' bracket, the radix sort's key width, k_seg_heads / collect_families
at the family boundary, the piece cuts at 256 records and 8 IMU factors, the near / far / heavy classes of the gather, the IMU
selection and its refusals, the share() split of the sharded form) on the planted windows of tests/window_cases.py, each of which
tests/test_window_cases_ref.py shows to be live on the CPU.

An accepted case is built and must return the case's (nb, nu, ni, pieces) - the piece count is the only way a wrong bracket at a
sample time shows when f == 0 makes both brackets the same function - and then meets linearize_ref.check_linearization at x = 0
and at a random point: H, g and the cost entry by entry in each entry's own scale under the bars that module derives per case from
the oracle's own floor (no tolerance of this file), residuals by class, exact symmetry, exact zero rows, the 3 x 3 structure.  A
refused case must return its code, leave the context unbuilt, and not disturb the build behind it.  A run with -s prints the
measured errors per case and the worst of them."""
import threading

import numpy as np
import pytest

import linearize_ref as lr
import window_cases as wc
from test_linearize_gpu import _build, _device

pytestmark = pytest.mark.gpu

LOG = []
WC_ERR_ARG = 11


@pytest.fixture(scope="module")
def ctx(gpu, oracle):
    c = gpu
    yield c
    c.set_params(oracle.default_params())
    rows = [r for r in LOG if r[2] is not None]
    for where, ns, floor, e, allow, bar in rows:  # (shown by a run with -s)
        print("%-44s floor eH %.1e eg %.1e cost %.1e | device eH %.1e eg %.1e cost %.1e" % (where, floor["eH"], floor["eg"], floor["ec"], e["eH"], e["eg"], e["ec"]))
    if rows:
        print("worst device eH %.2e eg %.2e cost %.2e over %d linearisations" % (max(r[3]["eH"] for r in rows), max(r[3]["eg"] for r in rows), max(r[3]["ec"] for r in rows), len(rows)))


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _solve_matches(c, W, ns):
    """the assertions of test_window_gpu.py::test_tiny_windows_match_oracle"""
    x0 = np.zeros(12 * ns)
    x_ref, s_ref, first_ref = W.solve(x0)
    x, s, first = c.window_solve(x0)
    assert s.termination == s_ref.termination and s.iterations == s_ref.iterations and s.successful_steps == s_ref.successful_steps, (
        s.termination, s_ref.termination, s.iterations, s_ref.iterations, s.successful_steps, s_ref.successful_steps)
    assert abs(s.final_cost - s_ref.final_cost) <= 1e-8 * s_ref.final_cost, (s.final_cost, s_ref.final_cost)
    assert _rel(first, first_ref) <= 1e-6 and _rel(x, x_ref) <= 1e-6, (_rel(first, first_ref), _rel(x, x_ref))


@pytest.mark.parametrize("name", wc.names(lambda c: c["rc"] == 0 and sum(c["shape"])))
def test_accepted_case(ctx, oracle, name):
    case = wc.by_name(oracle.default_params(), name)
    sp = case["sp"]
    ns = len(sp["w"]["sample_times"])
    keep = _build(ctx, sp)
    assert tuple(ctx.window_counts()) == case["shape"], (case["desc"], ctx.window_counts(), case["shape"])
    W = lr.oracle_window(oracle, sp)
    assert W.counts() == case["counts"]
    res = _device(ctx, ns, 1 + len(name))
    lr.check_linearization(oracle, sp, res, name, W=W, log=LOG)
    if name in ("kind-plus2", "kind-plus3"):
        # block pair (sp1l, sp2l + 1): all of the 12 x 12 block may be written while it is two blocks apart, the 6 x 6 pose corner
        # only - exact zeros around it - at three
        _, s1, s2, _, _, _ = case["lidar"][0]
        for r in res:
            blk = r["H"][12 * s1:12 * s1 + 12, 12 * (s2 + 1):12 * (s2 + 1) + 12]
            assert blk[:6, :6].any() and not blk[6:, :].any() and not blk[:, 6:].any(), name
        assert np.array_equal(lr.subblock_nonzero(res[1]["H"]), wc.expected_sparsity(case)), name
    if case["solve"]:
        _solve_matches(ctx, W, ns)
    del keep


def test_window_without_factors(ctx, oracle):
    """no pair and no IMU state: the build succeeds with zero pieces; H, g, the cost and the evaluation are exact zeros"""
    case = wc.by_name(oracle.default_params(), "family-empty")
    sp = case["sp"]
    ns = len(sp["w"]["sample_times"])
    keep = _build(ctx, sp)
    assert tuple(ctx.window_counts()) == (0, 0, 0, 0)
    for x in (np.zeros(12 * ns), lr.random_point(ns, 4)):
        H, g, cost = ctx.window_linearize(x)
        assert not H.any() and not g.any() and cost == 0.0
        assert ctx.window_evaluate(x) == 0.0
    del keep


def test_permuted_lists_build_the_same_bytes(ctx, oracle):
    """the radix sort is stable and every sum of the linearisation follows the sorted order (the original index of a record only
    addresses its residual - DESIGN.md 3.4): lists permuted so that the order within every key is kept give byte-equal H, g and
    cost, and the same residuals behind the permutation"""
    sp, sp_p, pb, pu = wc.permutation_pair(oracle.default_params())
    ns = len(sp["w"]["sample_times"])
    out = []
    for s in (sp, sp_p):
        keep = _build(ctx, s)
        out.append((_device(ctx, ns, 2), ctx.window_counts()))
        del keep
    (a, ca), (b, cb) = out
    assert ca == cb
    nb, nu = len(pb), len(pu)
    for ra, rb in zip(a, b):
        assert np.array_equal(ra["H"], rb["H"]) and np.array_equal(ra["g"], rb["g"]) and ra["cost"] == rb["cost"] and ra["eval_cost"] == rb["eval_cost"]
        assert np.array_equal(rb["res"][:nb], ra["res"][:nb][pb]) and np.array_equal(rb["res"][nb:nb + nu], ra["res"][nb:nb + nu][pu])
        assert np.array_equal(rb["res"][nb + nu:], ra["res"][nb + nu:])
    lr.check_linearization(oracle, sp, a, "permutation (original)", log=LOG)


@pytest.fixture(scope="module")
def good(oracle):
    """a good case and the bytes a fresh context gives for it"""
    from wildcat_slam_amd import lib

    case = wc.by_name(oracle.default_params(), "kind-plus1")
    ns = len(case["sp"]["w"]["sample_times"])
    fresh = lib.Context(0)
    try:
        keep = _build(fresh, case["sp"])
        ref = fresh.window_linearize(lr.random_point(ns, 8))
        del keep
    finally:
        fresh.close()
    return case, ref


@pytest.mark.parametrize("name", wc.names(lambda c: c["rc"] != 0))
def test_refused_case(ctx, oracle, good, name):
    from wildcat_slam_amd import lib

    case = wc.by_name(oracle.default_params(), name)
    ns = len(case["sp"]["w"]["sample_times"])
    with pytest.raises(lib.WildcatError) as e:
        _build(ctx, case["sp"])
    assert e.value.code == case["rc"], (case["desc"], str(e.value))
    if name.startswith("imucheck") and name != "imucheck-all-at-last":  # the message names the stamps
        assert "IMU triple" in str(e.value) and any("%.9f" % t in str(e.value) for t in case["sp"]["imu"]["t"]), str(e.value)
    with pytest.raises(lib.WildcatError) as e:  # not built
        ctx.window_linearize(np.zeros(12 * ns))
    assert e.value.code == WC_ERR_ARG
    ok, (H_ref, g_ref, c_ref) = good  # right behind the refusal: what a fresh context gives
    keep = _build(ctx, ok["sp"])
    assert tuple(ctx.window_counts()) == ok["shape"]
    H, g, c = ctx.window_linearize(lr.random_point(len(ok["sp"]["w"]["sample_times"]), 8))
    assert np.array_equal(H, H_ref) and np.array_equal(g, g_ref) and c == c_ref, case["desc"]
    del keep


@pytest.mark.parametrize("ns", [1, 341])
def test_sample_state_count_out_of_range(ctx, oracle, ns):
    from wildcat_slam_amd import lib

    case = wc.by_name(oracle.default_params(), "kind-plus1")
    sp = dict(case["sp"])
    sp["w"] = dict(sp["w"])
    sp["w"]["sample_times"] = sp["w"]["sample_times"][0] + 0.005 * np.arange(ns)
    with pytest.raises(lib.WildcatError) as e:
        _build(ctx, sp)
    assert e.value.code == WC_ERR_ARG


def _ranks(world, body, timeout=20.0):
    """body(rank, ctx, shared) on `world` thread-ranks with a ThreadComm each; no rank may wait for another that has left: a rank
    still alive after `timeout` fails the test (the barrier is then broken to release it)"""
    from wildcat_slam_amd import dist as wdist
    from wildcat_slam_amd import lib

    ctxs = [lib.Context(0) for _ in range(world)]
    shared = wdist.ThreadComm.shared(world)
    out, errors = [None] * world, [None] * world

    def run(r):
        try:
            ctxs[r].set_comm(wdist.ThreadComm(shared, r, ctxs[r]))
            out[r] = body(r, ctxs[r], shared)
        except Exception as e:
            errors[r] = e

    th = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=timeout)
    stuck = [r for r, t in enumerate(th) if t.is_alive()]
    if stuck:
        shared["bar"].abort()
        for t in th:
            t.join(timeout=5.0)
    try:
        assert not stuck, ("ranks still waiting", stuck, errors)
    finally:
        if not any(t.is_alive() for t in th):
            for c in ctxs:
                c.close()
    return out, errors


@pytest.mark.parametrize("option", [None, ("lm_one_collective", 1)])
@pytest.mark.parametrize("n_binary", [2, 3, 4])
def test_sharded_build_with_empty_shares(ctx, oracle, n_binary, option):
    """three thread-ranks, world - 1, world and world + 1 binary pairs and one unary pair: with two binary pairs rank 0's shares of
    both lists are empty.  Ranks bitwise equal, H, g and the cost under the reference's bars, the solve in the one-rank solve's
    iterations - in the default two-collective form and with lm_one_collective."""
    case = wc.sharded(oracle.default_params(), n_binary)
    sp = case["sp"]
    ns = len(sp["w"]["sample_times"])
    keep = _build(ctx, sp)
    assert tuple(ctx.window_counts()) == case["shape"]
    x_ref, s_ref, _ = ctx.window_solve(np.zeros(12 * ns))
    del keep

    def body(r, c, shared):
        if option:
            c.set_dev_option(*option)
        k = _build(c, sp, sharded=True)
        counts = c.window_counts()
        res = _device(c, ns, 9, residuals=False)
        for o in res:
            o["eval_cost"] = c.window_evaluate(o["x"])
        return counts, res, c.window_solve(np.zeros(12 * ns)), k

    out, errors = _ranks(3, body)
    assert not any(errors), errors
    nb_r = [o[0][0] for o in out]
    nu_r = [o[0][1] for o in out]
    assert sum(nb_r) == n_binary and sum(nu_r) == 1 and nb_r == [(n_binary * (r + 1)) // 3 - (n_binary * r) // 3 for r in range(3)]
    if n_binary == 2:
        assert nb_r[0] == 0 and nu_r[0] == 0  # a rank without a surfel factor
    for r in (1, 2):
        for a, b in zip(out[0][1], out[r][1]):
            assert np.array_equal(a["H"], b["H"]) and np.array_equal(a["g"], b["g"]) and a["cost"] == b["cost"] and a["eval_cost"] == b["eval_cost"], "ranks diverged"
        assert np.array_equal(out[0][2][0], out[r][2][0]), "ranks diverged in the solve"
    lr.check_linearization(oracle, sp, out[0][1], "%s %s" % (case["name"], "one collective" if option else "two collectives"), log=LOG)
    x, s, _ = out[0][2]
    assert s.iterations == s_ref.iterations and s.successful_steps == s_ref.successful_steps
    assert _rel(x, x_ref) < 1e-6


def test_sharded_refusal_in_one_rank_ends_every_rank(ctx, oracle):
    """three binary pairs on three ranks, the second one - rank 1's whole share - with t2 == times[ns-1]: rank 1 returns RANGE, the
    others fail the share check (its poisoned share), and none waits in a collective"""
    from wildcat_slam_amd import lib

    case = wc.sharded(oracle.default_params(), 3, defect_at=1)

    def body(r, c, shared):
        try:
            _build(c, case["sp"], sharded=True)
        except lib.WildcatError as e:
            return e.code
        return 0

    out, errors = _ranks(3, body)
    assert not any(errors), errors
    assert out[1] == wc.RANGE and out[0] == WC_ERR_ARG and out[2] == WC_ERR_ARG, out
