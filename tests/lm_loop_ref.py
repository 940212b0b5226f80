"""Ceres' trust-region Levenberg-Marquardt loop as the window solve runs it (oracle/window.cc: wco_window_solve; csrc/window.hip:
wc_window_solve), restated in float64 numpy around two callbacks, and the scenarios the loop is tested on.

The loop keeps all n = 12 ns unknowns (the rows the gauge zeroes come out as a zero step) and takes each step from
lm_step_ref.damped_system / solve (Cholesky refined on the Dot2 residual), so its decisions rest on a step at rounding level.  It
returns a TRACE - one record per iteration, with the two tolerance ratios and rho the decision was taken on - next to the summary the
solvers return.  margin(trace) says how far the closest decision of a solve sat from flipping: a scenario is fit for comparing
iteration counts only where that margin is far above what rounding moves."""
from collections import namedtuple

import numpy as np

import lm_step_ref as step_ref

ACCEPTED, REJECTED, INVALID, PARAMETER_TOLERANCE, FUNCTION_TOLERANCE = "+", "-", "x", "P", "F"

# kind: one of the five above; radius: the one the step was taken at; rho, step_ratio = step_norm / (1e-8 (|x| + 1e-8)), cost_ratio =
# |cost_change| / (1e-6 cost): None where the loop did not get to them; cost, x: the best point after the iteration (what a solve cut
# by max_iterations here returns)
Record = namedtuple("Record", "kind radius rho step_ratio cost_ratio cost x")
Summary = namedtuple("Summary", "iterations successful_steps unsuccessful_steps termination n_linearizations initial_cost final_cost x")


def lm_loop(linearize, evaluate, x0, radius0=1e4, max_iterations=50, refine=3):
    """linearize(x) -> H, g, cost; evaluate(x) -> cost.  -> (trace, summary).  termination: 0 converged, 1 cut by max_iterations,
    2 five invalid steps in a row"""
    x = np.array(x0, np.float64)
    H, g, cost = linearize(x)
    scale = 1.0 / (1.0 + np.sqrt(np.diag(H)))  # (Jacobi scaling: fixed at the first linearisation)
    initial_cost = min_cost = cost
    best = x.copy()
    x_norm = np.linalg.norm(x)
    radius, decrease = float(radius0), 2.0
    it = good = bad = invalid_run = 0
    n_lin, termination = 1, 1
    trace = []

    def done():
        return trace, Summary(it, good, bad, termination, n_lin, initial_cost, min_cost, best.copy())

    if np.abs(g).max() <= 1e-10:  # GradientToleranceReached before any step
        termination = 0
        return done()
    while True:
        if it >= max_iterations:
            termination = 1
            break
        if np.abs(g).max() <= 1e-10 or radius <= 1e-32:
            termination = 0
            break
        it += 1
        # LevenbergMarquardtStrategy::ComputeStep
        A, gs, _ = step_ref.damped_system(H, g, radius, scale)
        Hs = H * scale[:, None] * scale[None, :]
        try:
            with np.errstate(all="ignore"):
                y = step_ref.solve(A, gs, refine)
            model_change = float(y @ gs - 0.5 * (y @ (Hs @ y)))
            ok = bool(np.all(np.isfinite(y))) and model_change > 0
        except np.linalg.LinAlgError:
            ok = False
        if not ok:  # HandleInvalidStep
            invalid_run += 1
            trace.append(Record(INVALID, radius, None, None, None, min_cost, best.copy()))
            if invalid_run >= 5:  # (max_num_consecutive_invalid_steps; the fifth is not counted as a step)
                termination = 2
                break
            radius *= 0.5
            bad += 1
            continue
        invalid_run = 0
        cand = x - scale * y
        cand_cost = evaluate(cand)
        step_ratio = float(np.linalg.norm(x - cand) / (1e-8 * (x_norm + 1e-8)))
        if step_ratio <= 1.0:  # ParameterToleranceReached
            trace.append(Record(PARAMETER_TOLERANCE, radius, None, step_ratio, None, min_cost, best.copy()))
            termination = 0
            break
        cost_change = cost - cand_cost
        cost_ratio = float(abs(cost_change) / (1e-6 * cost))
        if cost_ratio <= 1.0:  # FunctionToleranceReached
            trace.append(Record(FUNCTION_TOLERANCE, radius, None, step_ratio, cost_ratio, min_cost, best.copy()))
            termination = 0
            break
        rho = cost_change / model_change
        taken_at = radius
        if rho > 1e-3:  # HandleSuccessfulStep
            x = cand
            x_norm = np.linalg.norm(x)
            H, g, cost = linearize(x)
            n_lin += 1
            radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            decrease = 2.0
            good += 1
            if cost < min_cost:
                min_cost, best = cost, x.copy()
            trace.append(Record(ACCEPTED, taken_at, rho, step_ratio, cost_ratio, min_cost, best.copy()))
        else:  # HandleUnsuccessfulStep
            radius /= decrease
            decrease *= 2.0
            bad += 1
            trace.append(Record(REJECTED, taken_at, rho, step_ratio, cost_ratio, min_cost, best.copy()))
    return done()


def trajectory(trace):
    return "".join(r.kind for r in trace)


def margin(trace):
    """the smallest distance of any decision of the solve from flipping: |log10| of each tolerance ratio tested, and
    |rho - 1e-3| / max(|rho|, 1e-3) of each acceptance test (inf for a trace without decisions)"""
    m = np.inf
    for r in trace:
        for ratio in (r.step_ratio, r.cost_ratio):
            if ratio is not None:
                m = min(m, abs(np.log10(ratio)) if ratio > 0 else np.inf)
        if r.rho is not None:
            m = min(m, abs(r.rho - 1e-3) / max(abs(r.rho), 1e-3))
    return float(m)


def prefix(trace, k, x0, initial_cost):
    """what a solve cut by max_iterations = k returns: (iterations, successful, unsuccessful, best cost, best x)"""
    head = trace[:k]
    good, bad = sum(r.kind == ACCEPTED for r in head), sum(r.kind in (REJECTED, INVALID) for r in head)
    return len(head), good, bad, (head[-1].cost if head else initial_cost), (head[-1].x if head else np.asarray(x0, np.float64))


def longest_rejected_run_before_acceptance(trace):
    t, best = trajectory(trace), 0
    for i, c in enumerate(t):
        if c == ACCEPTED and i and t[i - 1] == REJECTED:
            j = i
            while j and t[j - 1] == REJECTED:
                j -= 1
            best = max(best, i - j)
    return best


SWITCH = 1e7  # 10^lm_dense_radius: above it the default form takes the dense step


def expected_retries(prob, trace, form, upto=None):
    """dense re-tries: the rejected iterations that came from the elimination - the default form, four sample states or more, a
    radius at or below the switch"""
    if form != "default" or prob["ns"] < 4:
        return 0
    return sum(r.kind == REJECTED and r.radius <= SWITCH for r in trace[:upto])


def last_rejection(trace):
    """1-based iteration of the last rejected (or invalid) step, 0 if none"""
    return max([i + 1 for i, r in enumerate(trace) if r.kind in (REJECTED, INVALID)] or [0])


# ---- the scenarios (CPU only: synth + the oracle's matcher), shared by tests/test_lm_loop_ref.py and tests/test_lm_loop_gpu.py --------
# name: (n_scans, patches, fixed_patches, sample_dt or None for synth's default, seed, pose_err or None, fix_first, radius0 exponent).
# All with IMU factors: without them the bias block is damping only, which steps are invalid at a large radius depends on rounding,
# and numpy and the oracle already disagree about the trace (69 against 77 iterations on one such window).
Scenario = namedtuple("Scenario", "n_scans patches fixed sample_dt seed pose_err fix_first radius_exp")
SCENARIOS = {
    # 14 sample states
    "s11": Scenario(2, 150, 50, None, 11, None, 0, 4),
    "s13": Scenario(2, 150, 50, None, 13, None, 0, 4),
    "s13_gauge_03": Scenario(2, 150, 50, None, 13, (0.3, 0.02), 1, 4),
    "s11_06": Scenario(2, 150, 50, None, 11, (0.6, 0.05), 0, 4),
    "s13_gauge_06": Scenario(2, 150, 50, None, 13, (0.6, 0.05), 1, 4),
    "s12_gauge_06_r10": Scenario(2, 150, 50, None, 12, (0.6, 0.05), 1, 10),
    # 3 sample states: the dense step of all unknowns (the bias elimination needs four)
    "ns3_s24": Scenario(2, 150, 50, 0.6, 24, None, 0, 4),
    "ns3_s2_gauge": Scenario(2, 150, 50, 0.6, 2, None, 1, 4),
    # 65 sample states: 33 super-blocks, six levels of the cyclic reduction, an odd count (a phantom identity super-block)
    "ns65_s2_03": Scenario(8, 40, 15, 4.0 / 63.5, 2, (0.3, 0.02), 0, 4),
}


def scenario_problem(oracle, name, max_iterations=None):
    """-> dict(w, params, pairs, pf, fix_first, imu, ns, x0, radius0) of a scenario (lm_step_ref.oracle_window builds the oracle's)"""
    from wildcat_slam_amd import synth

    sc = SCENARIOS[name]
    kw = dict(seed=sc.seed, fixed_patches=sc.fixed)
    if sc.sample_dt is not None:
        kw["sample_dt"] = sc.sample_dt
    if sc.pose_err is not None:
        kw["pose_err"] = sc.pose_err
    w = synth.surfel_window(sc.n_scans, sc.patches, **kw)
    params = oracle.default_params()
    pairs = oracle.match(w["surf"], w["pose"], w["surf"], w["pose"], True, params)
    pf = oracle.match(w["surf"], w["pose"], w["fix_surf"], w["fix_pose"], False, params)
    if max_iterations is not None:
        params.max_iterations = max_iterations
    ns = len(w["sample_times"])
    return dict(w=w, params=params, pairs=pairs, pf=pf, fix_first=bool(sc.fix_first), imu=w["imu"], ns=ns, x0=np.zeros(12 * ns),
                radius0=10.0 ** sc.radius_exp)


# max |x_numpy - x_oracle| / max |x_oracle|, the worst over the states after every iteration (the end of the solve included),
# measured (tests/test_lm_loop_ref.py: the table of its docstring): the reference's own noise.  At radius0 = 1e10, which the oracle
# cannot run: the numpy loop with against without the refinement.
REF_DISTANCE = {"s11": 1.2e-12, "s13": 2.5e-13, "s13_gauge_03": 2.0e-8, "s11_06": 6.3e-9, "s13_gauge_06": 1.2e-8,
                "s12_gauge_06_r10": 2.9e-8, "ns3_s24": 6.8e-11, "ns3_s2_gauge": 7.8e-12, "ns65_s2_03": 1.5e-11}


def x_bar(name):
    """the device tests' bar on rel(x, x_reference): the 1e-6 of the existing solve tests (tests/test_window_gpu.py), or 10 x the
    reference's own noise where that is more - the loop amplifies rounding differences over tens of iterations"""
    return max(1e-6, 10.0 * REF_DISTANCE[name])


COST_BAR = 1e-8  # on |final_cost - reference| / reference, as the existing solve tests


def poisoned_problem(oracle, name="s11"):
    """a scenario's window with ONE value poisoned after the pairs were formed: the first centre coordinate of a fixed surfel that a
    unary pair uses is NaN.  Every linearisation then has a NaN cost, H and g: five invalid steps in a row, termination 2"""
    prob = scenario_problem(oracle, name)
    assert len(prob["pf"]) > 0
    prob["w"]["fix_surf"]["center"][prob["pf"]["first"][0], 0] = np.nan
    return prob


def with_max_iterations(prob, k):
    """the same problem under params.max_iterations = k (a copy: the oracle's window keeps the parameters it was made with)"""
    p = dict(prob)
    p["params"] = type(prob["params"]).from_buffer_copy(prob["params"])
    p["params"].max_iterations = int(k)
    return p


_REFERENCE = {}


def reference(oracle, name):
    """-> (problem, trace, summary) of a scenario by the numpy loop on the oracle's linearize / evaluate; computed once per
    process and shared (nobody writes to it)"""
    if name not in _REFERENCE:
        prob = scenario_problem(oracle, name)
        W = step_ref.oracle_window(oracle, prob)
        trace, summary = lm_loop(W.linearize, W.evaluate, prob["x0"], prob["radius0"], prob["params"].max_iterations)
        _REFERENCE[name] = (prob, trace, summary)
    return _REFERENCE[name]


def rel(a, b):
    """max |a - b| / max |b|: the measure the solve tests of tests/test_window_gpu.py put their 1e-6 on"""
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


def zero_residual_window(ns=6, per_state=8, seed=3):
    """a window whose every residual is exactly 0 at x = 0: identity poses, every pair joins a surfel to a byte-identical copy of
    itself under a later stamp, no IMU factors.  -> dict(surf, pose, pairs, sample_times, grav)"""
    from wildcat_slam_amd import records as R
    from wildcat_slam_amd import synth

    src = synth.surfel_window(2, 4 * per_state * ns, seed=seed)["surf"]
    times = 100.0 + 0.25 * np.arange(ns)
    rng = np.random.default_rng(seed)
    m = per_state * (ns - 1)
    t1 = np.sort(times[0] + 0.01 + (times[-1] - times[0] - 0.02) * rng.random(m))
    surf = np.concatenate([src[:m], src[:m]])
    surf["t"][:m] = t1
    # the copy: a later stamp inside the window, every other byte the same
    surf["t"][m:] = t1 + (times[-1] - 0.005 - t1) * (0.2 + 0.8 * rng.random(m))
    pose = np.zeros(2 * m, R.POSE)
    pose["quat"][:, 0] = 1.0
    pairs = np.zeros(m, R.PAIR)
    pairs["first"], pairs["second"] = np.arange(m), m + np.arange(m)
    a, b = surf[:m].copy(), surf[m:].copy()
    a["t"] = b["t"] = 0.0
    assert a.tobytes() == b.tobytes() and np.all(surf["t"][:m] < surf["t"][m:])
    return dict(surf=surf, pose=pose, pairs=pairs, sample_times=times, grav=np.array([0.0, 0.0, -9.81]))
