"""The window factors on the device away from the reference's default parameters, and the parameters nothing can run with.

Factors.  wc_window_linearize and wc_window_evaluate under every case of tests/window_params_cases.py - surfel_sigma0 0.05 and 1e-3,
cauchy_a 0.05 (most surfel factors deep in the loss's tail) and 50 (no matched factor reaches it), imu_dt 0.0025 and 0.01, each IMU
weight scaled alone, and everything together - on the default family's window at 8 sample states and on the six-mode window with the
reference's quirks and without, at x = 0 and at a random point: H, g, the cost and the residuals by class, by
linearize_ref.check_linearization unchanged - its bars and allowances are functions of the case's parameters, nothing is set by hand.
The correspondences stay those of the default matcher parameters.  tests/test_window_params_ref.py shows on the CPU that each case is
live: the oracle under the DEFAULT parameters misses these very bars by a factor of 4.5e3 (w_acc / 3, b2 x b2) to 1e14 in every
sub-block the parameter reaches, so a kernel with 200.0 for 1 / imu_dt, 0.16 for the loss or one weight in another's place fails here.
Measured on the MI355X (worst of the three windows and both points; floor = the oracle's sequential sums against the short-sum reference;
a run with -s prints every line, DESIGN.md 4.2 has the bars next to them):

    case                   floor eH / eg / cost            device eH / eg / cost           bar pose x pose, bias pairs
    surfel_sigma0 0.05     2.4e-15 / 4.0e-16 / 5.1e-16     2.3e-14 / 8.2e-15 / 2.0e-14     1.4e-12, 8.0e-14
    surfel_sigma0 1e-3     3.3e-15 / 9.0e-17 / 3.5e-16     2.3e-13 / 1.4e-14 / 1.3e-14     6.4e-11, 1.0e-13
    cauchy_a 0.05          2.6e-15 / 1.6e-16 / 1.8e-15     2.4e-12 / 1.8e-14 / 6.3e-15     6.1e-11, 8.4e-14
    cauchy_a 50            3.7e-15 / 3.3e-16 / 5.9e-16     4.1e-14 / 9.3e-15 / 6.5e-15     1.7e-13, 1.2e-13
    imu_dt 0.0025          2.2e-15 / 7.3e-17 / 3.5e-16     1.3e-13 / 4.5e-15 / 2.1e-15     7.7e-12, 8.0e-14
    imu_dt 0.01            3.2e-15 / 1.2e-16 / 7.6e-16     1.6e-13 / 7.7e-15 / 6.3e-15     7.7e-12, 1.0e-13
    w_gyr x 3              2.4e-15 / 2.7e-16 / 1.1e-15     1.1e-13 / 1.2e-14 / 1.5e-14     7.7e-12, 8.0e-14
    w_acc / 3              4.4e-15 / 2.8e-16 / 7.4e-16     1.5e-13 / 1.2e-14 / 1.5e-14     7.7e-12, 1.4e-13
    w_bg x 3, w_ba / 3     2.6e-15 / 1.8e-16 / 3.6e-16     1.5e-13 / 1.2e-14 / 1.5e-14     7.7e-12, 8.2e-14
    everything together    2.7e-15 / 3.0e-17 / 1.4e-16     1.1e-13 / 5.4e-15 / 6.7e-16     1.0e-11, 8.8e-14

(the device's largest eH sits in pose x pose; every type pair is asserted against its own bar).  No case failed; window.hip is unchanged.

Solve.  wc_window_solve against the oracle's solve at 8 sample states under "everything together" and under cauchy_a = 0.05, with the
assertions of test_window_gpu.py::test_lm_solve_matches_oracle.

When a parameter is read.  wc_window_build copies the factor parameters into the problem; wc_window_solve reads max_iterations when
it is called (include/wildcat_hip.h) - pinned by test_factor_parameters_are_read_at_the_build_and_max_iterations_at_the_solve.

Refusals.  Every value tests/test_params_check_cpu.py lists as refused is WC_ERR_ARG from wc_ctx_set_params, names its field, and
leaves the context as it was: the same extraction gives the same bytes on the same path before and after, a built window linearises
to the same bits.  No kernel-launching entry point is called while a refused value would be in force - it never is."""
import numpy as np
import pytest

import linearize_ref as lr
import window_params_cases as wp
from test_linearize_gpu import _build, _device
from test_params_check_cpu import RULES
from wildcat_slam_amd import lib

pytestmark = pytest.mark.gpu

LOG = []


@pytest.fixture(scope="module")
def ctx(gpu, oracle):
    """the suite's context; every test sets its own parameters, the defaults go back in at the end; a run with -s then prints floor,
    device value and bars per case"""
    yield gpu
    gpu.set_params(oracle.default_params())
    for where, ns, floor, e, allow, bar in LOG:
        if floor is None:
            print("%-56s %s" % (where, " ".join("%s %.1e/%.1e" % c_ for c_ in e)))
        else:
            print("%-56s floor eH %.1e eg %.1e cost %.1e | device eH %.1e eg %.1e cost %.1e | bars: bias pairs %.1e pose x pose %.1e rot x rot %.1e eg %.1e cost %.1e" % (
                where, floor["eH"], floor["eg"], floor["ec"], e["eH"], e["eg"], e["ec"], bar[0][2, 2], bar[0][1, 1], bar[0][0, 0], bar[1], bar[2]))


def _same_params(a, b):
    return bytes(a) == bytes(b)


@pytest.mark.parametrize("name", list(wp.CASES))
@pytest.mark.parametrize("which", wp.WINDOWS)
def test_factors_under_non_default_parameters(ctx, oracle, which, name):
    sp = wp.with_case(oracle, wp.window(oracle, which), name)
    keep = _build(ctx, sp)  # (sets sp's parameters on the context, then builds)
    assert _same_params(ctx.get_params(), sp["params"])
    W = lr.oracle_window(oracle, sp)
    cnt = W.counts()
    nb, nu, ni, _ = ctx.window_counts()
    assert (nb, nu, ni) == (cnt[0] + cnt[1] + cnt[2], cnt[3], cnt[4] + cnt[5])
    assert all(c > 0 for c in cnt) or which == "default ns=8"  # the six-mode window holds every factor mode
    lr.check_linearization(oracle, sp, _device(ctx, W.ns, 7), "%s, %s" % (which, name), W=W, log=LOG)
    del keep


def _solve_problem(oracle, name, max_iterations=100):
    sp = wp.with_case(oracle, lr.from_problem(lr.window_problem(oracle, 8, max_iterations=max_iterations)), name)
    assert sp["params"].max_iterations == max_iterations
    return sp


def _solve_matches(got, ref):
    """the assertions of test_window_gpu.py::test_lm_solve_matches_oracle"""
    from test_window_gpu import _rel

    (x, s, first), (x_ref, s_ref, first_ref) = got, ref
    assert s.termination == s_ref.termination and s.iterations == s_ref.iterations
    assert s.successful_steps == s_ref.successful_steps
    assert abs(s.initial_cost - s_ref.initial_cost) <= 1e-11 * s_ref.initial_cost
    assert abs(s.final_cost - s_ref.final_cost) <= 1e-8 * s_ref.final_cost
    # north_star: pose increments within 1e-6 relative
    assert _rel(first, first_ref) <= 1e-6, _rel(first, first_ref)
    assert _rel(x, x_ref) <= 1e-6, _rel(x, x_ref)
    return _rel(first, first_ref), _rel(x, x_ref)


@pytest.mark.parametrize("name", wp.SOLVE_CASES)
def test_solve_under_non_default_parameters(ctx, oracle, name):
    """the oracle: 31 iterations to convergence, the cost from 213 to 0.19, under everything together; under cauchy_a = 0.05 the full
    100 iterations, every one a successful step, without convergence (cost 1.17 to 0.90: deep in the loss's tail the steps are short).
    Measured on the MI355X, relative to the oracle (bar 1e-6): first step 5.2e-14 and corrections 2.6e-9; 8.7e-14 and 2.7e-10"""
    sp = _solve_problem(oracle, name)
    keep = _build(ctx, sp)
    x0 = np.zeros(12 * 8)
    ref = lr.oracle_window(oracle, sp).solve(x0)
    got = ctx.window_solve(x0)
    print("%s: iterations %d, termination %d, cost %.6g -> %.6g, first step and corrections against the oracle (relative): %.1e %.1e" % (
        (name, got[1].iterations, got[1].termination, got[1].initial_cost, got[1].final_cost) + _solve_matches(got, ref)))
    assert ref[1].final_cost < ref[1].initial_cost and ref[1].iterations >= 30
    del keep


def test_factor_parameters_are_read_at_the_build_and_max_iterations_at_the_solve(ctx, oracle):
    """build under set A (everything together); wc_ctx_set_params(B) - B = the defaults with max_iterations = 3; the linearisation,
    the evaluation and the solve's factors are A's (B's reference is missed by the factors tests/test_window_params_ref.py measures),
    the solve's iteration limit is B's"""
    spA = _solve_problem(oracle, "everything together")
    keep = _build(ctx, spA)
    B = oracle.default_params()
    B.max_iterations = 3
    ctx.set_params(B)
    assert _same_params(ctx.get_params(), B)
    W = lr.oracle_window(oracle, spA)
    results = _device(ctx, 8, 7)
    lr.check_linearization(oracle, spA, results, "built under A, linearised under B", W=W)
    spB = dict(spA, params=B)
    with pytest.raises(AssertionError):
        lr.check_linearization(oracle, spB, results, "B's reference", W=lr.oracle_window(oracle, spB))
    # the solve: A's factors, B's limit - the oracle with A's parameters and max_iterations = 3
    spA3 = _solve_problem(oracle, "everything together", max_iterations=3)
    x0 = np.zeros(12 * 8)
    ref = lr.oracle_window(oracle, spA3).solve(x0)
    got = ctx.window_solve(x0)
    _solve_matches(got, ref)
    assert got[1].iterations == 3 and got[1].termination == 1  # (under the 100 it was built with: 31 and convergence)
    # ... and back: the limit follows the next set_params again
    A = spA["params"]
    ctx.set_params(A)
    got = ctx.window_solve(x0)
    _solve_matches(got, lr.oracle_window(oracle, spA).solve(x0))
    assert got[1].iterations > 3 and got[1].termination == 0
    del keep


def _refused():
    """(field, value) of every refused value of tests/test_params_check_cpu.py, and the three view_point axes"""
    out = [(field, v) for field in sorted(RULES) for v in RULES[field][0]]
    return out + [(("view_point", axis), v) for axis in range(3) for v in (float("nan"), float("inf"), float("-inf"))]


def _refuse_all(ctx, oracle, base):
    """every refused value on top of `base`: WC_ERR_ARG each time, the field named, the context's parameters still base's"""
    n = 0
    for field, v in _refused():
        p = oracle.default_params()
        p.reference_quirks, p.max_iterations = base.reference_quirks, base.max_iterations
        if isinstance(field, tuple):
            p.view_point[field[1]] = v
            field = field[0]
        else:
            setattr(p, field, v)
        with pytest.raises(lib.WildcatError) as err:
            ctx.set_params(p)
        assert err.value.code == lib.WC_ERR_ARG and field in str(err.value), (field, v, str(err.value))
        assert _same_params(ctx.get_params(), base) and ctx.params is base, (field, v)
        n += 1
    return n


def test_refused_parameters_leave_the_extraction_as_it_was(ctx, oracle):
    from wildcat_slam_amd import synth

    base = oracle.default_params()
    ctx.set_params(base)
    pts, _ = synth.g2_lattice(120, m=40)
    ctx.extract_surfels(pts)  # (the first sweep after a set_params starts the adaptive path choice afresh; the second is the steady state)
    s0, id0 = ctx.extract_surfels(pts)
    info0 = ctx.extract_path_info()
    assert len(s0) > 100
    assert _refuse_all(ctx, oracle, base) >= 80
    assert ctx.extract_path_info() == info0  # (a refusal does not reset the path choice either)
    s1, id1 = ctx.extract_surfels(pts)
    assert s1.tobytes() == s0.tobytes() and id1.tobytes() == id0.tobytes()
    assert ctx.extract_path_info() == info0


def test_refused_parameters_leave_a_built_window_as_it_was(ctx, oracle):
    sp = wp.window(oracle, "six modes quirks=1")
    keep = _build(ctx, sp)
    base = sp["params"]
    _refuse_all(ctx, oracle, base)
    x = lr.random_point(len(sp["w"]["sample_times"]), 7)
    H0, g0, c0 = ctx.window_linearize(x)
    assert np.any(H0) and np.all(np.isfinite(H0)) and np.all(np.isfinite(g0)) and np.isfinite(c0)
    _refuse_all(ctx, oracle, base)
    H1, g1, c1 = ctx.window_linearize(x)
    assert np.array_equal(H0, H1) and np.array_equal(g0, g1) and c0 == c1
    lr.check_linearization(oracle, sp, _device(ctx, len(sp["w"]["sample_times"]), 7), "six modes quirks=1 after the refusals")
    del keep
