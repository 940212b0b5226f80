"""The trust-region loop of wc_window_solve (csrc/window.hip) on the device against the numpy loop of tests/lm_loop_ref.py, on windows
where steps are REJECTED - every other test of the solve runs windows on which almost every step is accepted.  The loop's hand-written
state (x / xc swapped on acceptance, the double-buffered {H, g, cost}, level 0 of the cyclic reduction formed speculatively from the
candidate's H, the dense re-try of a rejected elimination step, the radius / decrease recurrence, the switch to the dense step above a
radius of 1e7) is watched ITERATION BY ITERATION: a solve under max_iterations = k returns the best point after k iterations, so a
wrong buffer or radius after the j-th rejection shows at k = j + 1, not only as another end point.  Scenarios, their margins and the
reference's own noise: tests/test_lm_loop_ref.py.  Both forms of every scenario: the default and lm_dense = 1.

Branches and the cases that enter them:
    HandleSuccessfulStep                              every scenario, every prefix with a `+`
    HandleUnsuccessfulStep, `decrease` doubling       runs of 5 to 11 rejections (s11, s13, s13_gauge_03, s13_gauge_06, ns3_*, ns65_s2_03)
    HandleInvalidStep up to consecutive_invalid == 5  test_poisoned_window_fails_after_five_invalid_steps (termination 2)
    the dense re-try (summary.first_step[1])          every rejection at a radius <= 1e7 of the default form at 14 and 65 sample states
    the lm_dense_radius switch inside one solve       s12_gauge_06_r10 (radius0 = 1e10, down through 1e7 by rejections), ns65_s2_03 (up
                                                      through 1e7 by acceptances and down again)
    function / parameter tolerance                    every scenario's last iteration (`F`), s13_gauge_06 (`P`)
    the gradient tolerance before any step            test_zero_residual_window_stops_before_any_step
    max_iterations                                    every prefix, k = 0 included
    two_late (sharded, two collectives) and a
    rejected step                                     test_sharded_solve_with_rejections
    radius <= 1e-32                                   not reached on the device (a long run of rejections in a row, and the parameter
                                                      tolerance fires first): tests/test_lm_loop_cpu.py, on scripted mails - the
                                                      decisions are csrc/lm_loop.h's, which that file drives without a GPU

Bars: counts and termination exact; x within max(1e-6, 10 x the reference's own noise) in max |x - ref| / max |ref| (1e-6 is the bar
of the solve tests of tests/test_window_gpu.py; the noise, numpy against the oracle, is at most 2.9e-8, so the bar is 1e-6 on every
scenario); the cost within 1e-8 relative.  Measured on the MI355X, worst over the full solve and all prefixes, default / dense form:

    scenario           bar     default   lm_dense = 1
    s11                1e-6    2.5e-12   3.2e-12
    s13                1e-6    2.4e-13   4.1e-13
    s13_gauge_03       1e-6    7.5e-08   7.5e-08
    s11_06             1e-6    2.3e-08   2.8e-08
    s13_gauge_06       1e-6    5.7e-08   6.0e-08
    s12_gauge_06_r10   1e-6    2.0e-07   2.0e-07
    ns3_s24            1e-6    7.2e-10   7.2e-10
    ns3_s2_gauge       1e-6    4.2e-11   4.2e-11
    ns65_s2_03         1e-6    9.9e-11   1.0e-10
"""
import numpy as np
import pytest

import lm_loop_ref as ref

pytestmark = pytest.mark.gpu

DEFAULTS = {"lm_dense": 0, "lm_radius0": -1, "lm_dense_radius": 7}
FORMS = {"default": {}, "dense": {"lm_dense": 1}}
NAMES = tuple(ref.SCENARIOS)
WORST = {}


@pytest.fixture(scope="module")
def ctx():
    """a context of its own: the solves run under their own max_iterations and development options"""
    from wildcat_slam_amd import lib

    c = lib.Context(0)
    yield c
    if WORST:
        print("\nworst distance of x from the reference (full solve and prefixes), against its bar:")
        for name in NAMES:
            print("  %-18s bar %.1e  %s" % (name, ref.x_bar(name), "  ".join("%s %.1e" % (f, WORST[name, f]) for f in FORMS if (name, f) in WORST)))
    c.close()


def _build(ctx, prob, sharded=False):
    w = prob["w"]
    ctx.set_params(prob["params"])
    keep = [ctx.to_device(a) for a in (w["surf"], w["pose"], prob["pairs"], w["fix_surf"], w["fix_pose"], prob["pf"])]
    ctx.window_build(keep[0], keep[1], keep[2], len(prob["pairs"]), prob["imu"], w["sample_times"], w["grav"], prob["fix_first"], keep[3],
                     keep[4], keep[5], len(prob["pf"]), sharded=sharded)
    return keep


def _options(prob, form):
    opts = dict(FORMS[form])
    if prob["radius0"] != 1e4:
        opts["lm_radius0"] = int(round(np.log10(prob["radius0"])))
    return opts


def _solve(ctx, prob, opts, max_iterations=None):
    """the built window solved from x0 under max_iterations (None: the parameters' own) and the development options `opts`"""
    params = prob["params"] if max_iterations is None else ref.with_max_iterations(prob, max_iterations)["params"]
    try:
        ctx.set_params(params)
        for k, v in opts.items():
            ctx.set_dev_option(k, v)
        x, s, _ = ctx.window_solve(prob["x0"])
    finally:
        for k, v in DEFAULTS.items():
            ctx.set_dev_option(k, v)
        ctx.set_params(prob["params"])
    return x, s


def _counts(s):
    return s.iterations, s.successful_steps, s.unsuccessful_steps, s.termination


def _check_state(name, form, tag, x, s, want_counts, want_cost, want_x):
    assert _counts(s) == want_counts, (name, form, tag, _counts(s), want_counts)
    assert s.n_linearizations == 1 + s.successful_steps, (name, form, tag)
    if not np.any(want_x):
        assert x.tobytes() == want_x.tobytes(), (name, form, tag)
        d = 0.0
    else:
        d = ref.rel(x, want_x)
    WORST[name, form] = max(WORST.get((name, form), 0.0), d)
    assert d <= ref.x_bar(name), (name, form, tag, d, ref.x_bar(name))
    assert abs(s.final_cost - want_cost) <= ref.COST_BAR * want_cost, (name, form, tag, s.final_cost, want_cost)
    return d


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", NAMES)
def test_full_solve_follows_the_reference(ctx, oracle, name, form):
    prob, trace, want = ref.reference(oracle, name)
    keep = _build(ctx, prob)
    x, s = _solve(ctx, prob, _options(prob, form))
    d = _check_state(name, form, "full", x, s, _counts(want), want.final_cost, want.x)
    print("\n%-18s %-7s %s  iterations %d  distance %.1e (bar %.1e)  dense re-tries %d" % (name, form, ref.trajectory(trace), s.iterations, d,
                                                                                        ref.x_bar(name), s.first_step[1]))
    assert abs(s.initial_cost - want.initial_cost) <= 1e-11 * want.initial_cost
    assert want.unsuccessful_steps > 0 and s.unsuccessful_steps == want.unsuccessful_steps  # (rejections happened, on the device too)
    assert s.first_step[1] == ref.expected_retries(prob, trace, form), (name, form, s.first_step[1])
    del keep


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", NAMES)
def test_prefixes_follow_the_reference(ctx, oracle, name, form):
    """max_iterations = 0, and every k from 1 to two past the trace's last rejection: the counts of the trace's first k iterations,
    termination 1 while the solve is cut short, the best x and cost after k iterations"""
    prob, trace, want = ref.reference(oracle, name)
    keep = _build(ctx, prob)
    opts = _options(prob, form)
    last = ref.last_rejection(trace) + 2
    worst = 0.0
    for k in range(0, last + 1):
        x, s = _solve(ctx, prob, opts, k)
        if k < want.iterations:
            it, good, bad, cost, x_k = ref.prefix(trace, k, prob["x0"], want.initial_cost)
            worst = max(worst, _check_state(name, form, "k=%d" % k, x, s, (it, good, bad, 1), cost, x_k))
            assert s.first_step[1] == ref.expected_retries(prob, trace, form, k), (name, form, k, s.first_step[1])
        else:  # (past the trace's end: the whole solve)
            worst = max(worst, _check_state(name, form, "k=%d" % k, x, s, _counts(want), want.final_cost, want.x))
    print("\n%-18s %-7s prefixes 0..%d  worst distance %.1e (bar %.1e)" % (name, form, last, worst, ref.x_bar(name)))
    del keep


def test_zero_residual_window_stops_before_any_step(ctx, oracle):
    """identity poses, every pair a surfel and its byte-identical copy under a later stamp, no IMU factors: every residual is exactly
    0, max |g| = 0 <= 1e-10 at the first linearisation - termination 0 with no iteration, no step, x untouched"""
    z = ref.zero_residual_window()
    ctx.set_params(oracle.default_params())
    keep = [ctx.to_device(a) for a in (z["surf"], z["pose"], z["pairs"])]
    ctx.window_build(keep[0], keep[1], keep[2], len(z["pairs"]), None, z["sample_times"], z["grav"], True)
    x0 = np.zeros(12 * len(z["sample_times"]))
    for form in FORMS:
        prob = dict(params=oracle.default_params(), x0=x0)
        x, s = _solve(ctx, prob, FORMS[form])
        assert _counts(s) == (0, 0, 0, 0) and s.n_linearizations == 1, (form, _counts(s))
        assert x.tobytes() == x0.tobytes() and s.initial_cost == 0.0 and s.final_cost == 0.0, (form, s.initial_cost)
    del keep


def test_poisoned_window_fails_after_five_invalid_steps(ctx, oracle):
    """one centre coordinate of one fixed surfel that a unary pair uses is NaN (set after the pairs were formed).  The build and the
    factor kernels use a centre in arithmetic only - k_build_records rotates it into the record, k_pair_keys sorts by the stamps, no
    kernel of the solve waits on a value - so the NaN reaches the cost, H and g and nothing else: every step is invalid (the
    elimination's, and its dense re-try), five in a row end the solve as the oracle's does - termination 2 at iteration 5, four of
    them counted, x untouched.  Run once: an error path, not a stress loop."""
    prob = ref.poisoned_problem(oracle)
    keep = _build(ctx, prob)  # (the build looks at stamps and indices only: it does not refuse the window)
    x, s = _solve(ctx, prob, {})
    assert _counts(s) == (5, 0, 4, 2), _counts(s)
    assert s.n_linearizations == 1 and x.tobytes() == prob["x0"].tobytes()
    del keep


def test_sharded_solve_with_rejections(ctx, oracle):
    """the first scenario on two thread-ranks of one GPU in the default two-collective form (wc_window_build_sharded, the IMU factors
    on every rank): max |g| of an accepted point arrives one ticket late (two_late) - here next to rejected steps and their dense
    re-tries.  Both ranks: the one-rank solve's counts and termination, x within the scenario's bar"""
    import threading

    from wildcat_slam_amd import dist as wdist
    from wildcat_slam_amd import lib

    name = NAMES[0]
    prob, trace, want = ref.reference(oracle, name)
    keep = _build(ctx, prob)
    x_one, s_one = _solve(ctx, prob, {})
    assert _counts(s_one) == _counts(want) and want.unsuccessful_steps >= 5
    world = 2
    ctxs = [lib.Context(0) for _ in range(world)]
    shared = wdist.ThreadComm.shared(world)
    res, errors = [None] * world, []

    def run(r):
        try:
            c = ctxs[r]
            c.set_comm(wdist.ThreadComm(shared, r, c))
            k = _build(c, prob, sharded=True)
            assert c.window_reduce_bytes() == 8 * wdist.corner_count(prob["ns"])  # (the two-collective form's payload)
            res[r] = c.window_solve(prob["x0"]) + (k,)
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
        assert np.array_equal(res[0][0], res[1][0]), "ranks diverged"
        for r in range(world):
            x, s = res[r][0], res[r][1]
            assert _counts(s) == _counts(s_one), (r, _counts(s), _counts(s_one))
            assert s.n_linearizations == 1 + s.successful_steps
            d = ref.rel(x, x_one)
            assert d <= ref.x_bar(name) and ref.rel(x, want.x) <= ref.x_bar(name), (r, d)
            assert abs(s.final_cost - want.final_cost) <= ref.COST_BAR * want.final_cost
        print("\n%-18s two ranks %s  distance from the one-rank solve %.1e" % (name, ref.trajectory(trace), ref.rel(res[0][0], x_one)))
    finally:
        for c in ctxs:
            c.close()
    del keep
