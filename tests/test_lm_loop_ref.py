"""The reference of tests/test_lm_loop_gpu.py held on the CPU: the numpy trust-region loop (tests/lm_loop_ref.py) against the oracle's
solve (oracle/window.cc), iteration by iteration, and the conditions that make its scenarios worth running on the device.

Scenarios (lm_loop_ref.SCENARIOS; synth.surfel_window, pairs by the oracle's matcher, default parameters, IMU factors on all).
`+` accepted, `-` rejected, `F` / `P` the function / parameter tolerance; distance = max |x_numpy - x_oracle| / max |x_oracle| (numpy:
Cholesky refined on the Dot2 residual; the oracle: plain Cholesky) at the end of the solve, and the worst over the states after every
iteration (the prefixes) - the reference's own noise, from which the device test takes its bar (lm_loop_ref.REF_DISTANCE holds the
worst).  For the scenario at a radius of 1e10, which the oracle (1e4 hard-coded) cannot run, the distance is between the numpy loop
with and without the refinement.

    scenario           states  gauge  pose_err     radius0  trajectory                          margin  distance: end  worst
    s11                14      free   default      1e4      +++++++------++F                    0.24    1.2e-12        1.2e-12
    s13                14      free   default      1e4      ++++++------F                       0.37    2.2e-13        2.5e-13
    s13_gauge_03       14      held   (0.3, 0.02)  1e4      17 +, 7 -, F                        0.12    7.1e-11        2.0e-08
    s11_06             14      free   (0.6, 0.05)  1e4      +++++++++++++++-----+--+--+---++F   0.22    6.2e-09        6.3e-09
    s13_gauge_06       14      held   (0.6, 0.05)  1e4      54 +, 11 -, P  (66 iterations)      0.37    9.9e-10        1.2e-08
    s12_gauge_06_r10   14      held   (0.6, 0.05)  1e10     21 +, 9 -, +--F                     0.59    2.9e-10        2.9e-08
    ns3_s24            3       free   default      1e4      +++++++------+--+--F                0.49    6.8e-11        6.8e-11
    ns3_s2_gauge       3       held   default      1e4      ++++++------+-+--F                  0.62    7.8e-12        7.8e-12
    ns65_s2_03         65      free   (0.3, 0.02)  1e4      +++++++++------+-+-F                0.72    1.5e-11        1.5e-11

Found by searching seeds and pose_err under the conditions below: the 3-state windows among seeds 1 - 24 (35 of 144 windows reject a
step at all), the 65-state one among seeds 1 - 6 of windows of 8 sweeps x 40 patches (windows with 150 or more patches per sweep at 65
states never reject).  Windows WITHOUT IMU factors are left out wherever the reference's trace has an invalid step: their bias block
is damping only, which steps are invalid at a large radius depends on rounding, and numpy and the oracle disagree about the trace
themselves (69 against 77 iterations on one window)."""
import numpy as np
import pytest

import lm_loop_ref as ref
import lm_step_ref as step_ref

NAMES = tuple(ref.SCENARIOS)
ORACLE_NAMES = tuple(n for n in NAMES if ref.SCENARIOS[n].radius_exp == 4)  # (the oracle's initial radius is hard-coded)


def _counts(s):
    return s.iterations, s.successful_steps, s.unsuccessful_steps, s.termination


@pytest.mark.parametrize("name", ORACLE_NAMES)
def test_loop_matches_oracle(oracle, name):
    """same iterations, successful and unsuccessful steps and termination; the distance of the two end points is the docstring's"""
    prob, trace, s = ref.reference(oracle, name)
    x_o, s_o, _ = step_ref.oracle_window(oracle, prob).solve(prob["x0"])
    assert _counts(s) == _counts(s_o), (ref.trajectory(trace), _counts(s), _counts(s_o))
    assert s.n_linearizations == s_o.n_linearizations == 1 + s.successful_steps
    assert s.iterations == len(trace) and s.termination == 0
    d = ref.rel(s.x, x_o)
    print("%-18s %s margin %.2f distance %.1e" % (name, ref.trajectory(trace), ref.margin(trace), d))
    assert d <= 3 * ref.REF_DISTANCE[name], (d, ref.REF_DISTANCE[name])  # (the recorded figure is the measured one, not a stale one)
    assert abs(s.final_cost - s_o.final_cost) <= 1e-9 * s_o.final_cost


def test_refinement_distance_at_the_large_radius(oracle):
    """the scenario the oracle cannot run: the loop without the refinement takes the same decisions; its distance is the recorded one"""
    name = "s12_gauge_06_r10"
    prob, trace, s = ref.reference(oracle, name)
    W = step_ref.oracle_window(oracle, prob)
    trace_p, s_p = ref.lm_loop(W.linearize, W.evaluate, prob["x0"], prob["radius0"], prob["params"].max_iterations, refine=0)
    assert ref.trajectory(trace_p) == ref.trajectory(trace)
    d = max(ref.rel(a.x, b.x) for a, b in zip(trace, trace_p))  # (after every iteration, the last included)
    print("%-18s %s margin %.2f distance %.1e (end), %.1e (worst)" % (name, ref.trajectory(trace), ref.margin(trace), ref.rel(s.x, s_p.x), d))
    assert d <= 3 * ref.REF_DISTANCE[name], (d, ref.REF_DISTANCE[name])


@pytest.mark.parametrize("name", ORACLE_NAMES)
def test_prefix_property(oracle, name):
    """the oracle under max_iterations = k returns the trace's state after k iterations, for every k: counts, termination 1 while
    cut short, best x and cost - so a solver that only returns a summary can be watched iteration by iteration"""
    prob, trace, s = ref.reference(oracle, name)
    worst = 0.0
    for k in range(0, s.iterations + 2):
        x_k, s_k, _ = step_ref.oracle_window(oracle, ref.with_max_iterations(prob, k)).solve(prob["x0"])
        if k < s.iterations:
            it, good, bad, cost, x = ref.prefix(trace, k, prob["x0"], s.initial_cost)
            want = (it, good, bad, 1)
        else:
            want, cost, x = _counts(s), s.final_cost, s.x
        assert _counts(s_k) == want, (k, _counts(s_k), want)
        assert abs(s_k.final_cost - cost) <= 1e-9 * cost, (k, s_k.final_cost, cost)
        if k == 0:
            assert np.array_equal(x_k, prob["x0"]) and s_k.final_cost == s_k.initial_cost
        else:
            worst = max(worst, ref.rel(x, x_k))
    print("%-18s worst distance over the prefixes %.1e" % (name, worst))
    assert worst <= 3 * ref.REF_DISTANCE[name], (worst, ref.REF_DISTANCE[name])


def test_every_scenario_is_decided_clear_of_rounding(oracle):
    """conditions on the inputs, for the reference alone: no decision of any scenario within 0.05 of flipping, no invalid step"""
    for name in NAMES:
        _, trace, s = ref.reference(oracle, name)
        assert ref.margin(trace) >= 0.05, (name, ref.margin(trace))
        assert ref.INVALID not in ref.trajectory(trace), name
        assert s.iterations < 100 and s.unsuccessful_steps > 0, name


def _dense_switch_crossed_by_rejections(trace, switch=1e7):
    """a rejected step above the switch whose shrunken radius, at or below it, is the next step's: both sides in one solve"""
    return any(a.kind == ref.REJECTED and a.radius > switch >= b.radius for a, b in zip(trace, trace[1:]))


def test_scenarios_cover_the_loop(oracle):
    traces = {name: ref.reference(oracle, name)[1] for name in NAMES}
    t = {name: ref.trajectory(tr) for name, tr in traces.items()}
    assert any(ref.longest_rejected_run_before_acceptance(tr) >= 5 for tr in traces.values())
    assert any("+-+" in s or "-+-" in s for s in t.values())  # rejections interleaved with acceptances
    assert any(s.endswith("-F") for s in t.values())          # the function tolerance directly behind a rejection
    assert any(s.endswith("P") for s in t.values())           # the parameter tolerance
    r10 = [n for n in NAMES if ref.SCENARIOS[n].radius_exp == 10]
    assert r10 and any(_dense_switch_crossed_by_rejections(traces[n]) for n in r10)
    # `decrease` doubles: a second rejection in a row divides the radius by 4, a third by 8
    assert any(a.kind == b.kind == c.kind == ref.REJECTED and b.radius == a.radius / 2 and c.radius == b.radius / 4
               for tr in traces.values() for a, b, c in zip(tr, tr[1:], tr[2:]))
    # sizes: the all-dense path (fewer than four sample states), 14, and several levels of the cyclic reduction
    ns = {ref.reference(oracle, n)[0]["ns"] for n in NAMES}
    assert 3 in ns and 14 in ns and max(ns) >= 65


def _quadratic(H, b):
    H, b = np.asarray(H, float), np.asarray(b, float)
    return (lambda x: (H, H @ x - b, 0.5 * x @ H @ x - b @ x + 10.0)), (lambda x: 0.5 * x @ H @ x - b @ x + 10.0)


def test_loop_exits_without_the_oracle():
    """the exits no window scenario takes, on a quadratic: the gradient tolerance before any step, max_iterations, and five invalid
    steps in a row (termination 2 at iteration 5 with 4 of them counted, x untouched)"""
    lin, ev = _quadratic(np.diag([1.0, 4.0]), [1.0, 2.0])
    trace, s = ref.lm_loop(lin, ev, [1.0, 0.5])  # the minimum: g = 0
    assert trace == [] and (s.iterations, s.successful_steps, s.unsuccessful_steps, s.termination) == (0, 0, 0, 0)
    trace, s = ref.lm_loop(lin, ev, [0.0, 0.0], max_iterations=1)
    assert ref.trajectory(trace) == "+" and (s.iterations, s.successful_steps, s.termination) == (1, 1, 1)
    assert ref.prefix(trace, 1, [0.0, 0.0], s.initial_cost)[:3] == (1, 1, 0) and s.final_cost < s.initial_cost
    trace, s = ref.lm_loop(lin, ev, [0.0, 0.0], max_iterations=0)
    assert trace == [] and s.termination == 1 and np.array_equal(s.x, [0.0, 0.0])
    nan_lin = lambda x: (np.array([[1.0, 0.0], [0.0, np.nan]]), np.array([1.0, np.nan]), np.nan)
    trace, s = ref.lm_loop(nan_lin, ev, [0.25, 0.5])
    assert ref.trajectory(trace) == "xxxxx" and (s.iterations, s.successful_steps, s.unsuccessful_steps, s.termination) == (5, 0, 4, 2)
    assert [r.radius for r in trace] == [1e4 / 2 ** i for i in range(5)] and np.array_equal(s.x, [0.25, 0.5])
    assert ref.margin(trace) == np.inf


def test_margin_counts_what_a_record_tested():
    R = ref.Record
    x = np.zeros(1)
    assert ref.margin([R("+", 1e4, 0.5, 1e3, 1e2, 1.0, x)]) == pytest.approx(0.998)
    assert ref.margin([R("-", 1e4, -2e-3, 1e3, 1e2, 1.0, x)]) == pytest.approx(1.5)
    assert ref.margin([R("+", 1e4, 0.5, 10 ** 0.03, 1e2, 1.0, x)]) == pytest.approx(0.03)
    assert ref.margin([R("F", 1e4, None, 1e3, 10 ** -0.2, 1.0, x)]) == pytest.approx(0.2)
    assert ref.margin([R("P", 1e4, None, 10 ** -0.4, None, 1.0, x)]) == pytest.approx(0.4)  # (the cost ratio was never formed)


def test_zero_residual_window_stops_at_the_initial_gradient(oracle):
    """the hand-made window of the device test's gradient-tolerance case: every residual exactly 0, no iteration"""
    z = ref.zero_residual_window()
    W = oracle.Window(z["sample_times"], z["grav"], True, oracle.default_params())
    W.add_binary(z["surf"], z["pose"], z["pairs"])
    x0 = np.zeros(12 * len(z["sample_times"]))
    cost, res = W.evaluate(x0, want_residuals=True)
    assert len(res) == len(z["pairs"]) and not res.any() and cost == 0.0
    x, s, _ = W.solve(x0)
    assert (s.iterations, s.successful_steps, s.unsuccessful_steps, s.termination) == (0, 0, 0, 0) and x.tobytes() == x0.tobytes()
    assert set(W.counts()[:3]) != {0}


def test_poisoned_window_fails_after_five_invalid_steps(oracle):
    """the device test's failure case on the oracle: one centre coordinate of a fixed surfel a unary pair uses is NaN"""
    prob = ref.poisoned_problem(oracle)
    x, s, _ = step_ref.oracle_window(oracle, prob).solve(prob["x0"])
    assert (s.iterations, s.successful_steps, s.unsuccessful_steps, s.termination) == (5, 0, 4, 2) and x.tobytes() == prob["x0"].tobytes()
