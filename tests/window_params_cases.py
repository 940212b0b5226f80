"""The window factors away from their default parameters: the cases and windows shared by tests/test_window_params_ref.py (CPU: every
case is live, the two loss cases are the regimes they claim) and tests/test_window_params_gpu.py (the device against the short-sum
reference of tests/linearize_ref.py under each case's parameters).

Every case changes one thing from oracle.default_params() and one changes all of them.  The correspondences of a window are those of
the default matcher parameters in every case, so only the factors change.  REACH names, per case, unknown-type pairs (rows / columns
rot, pos, b1 = gyroscope bias, b2 = accelerometer bias) whose H entries the parameter scales: where a device that ignored the parameter
must leave check_linearization's bar behind."""
import numpy as np

import linearize_ref as lr

ROT, POS, B1, B2 = range(4)


def _scale(name, factor):
    def f(p):
        setattr(p, name, getattr(p, name) * factor)
    return f


def _set(name, value):
    def f(p):
        setattr(p, name, value)
    return f


def _all(p):
    for name in SINGLE:
        if name not in ("surfel_sigma0 1e-3", "cauchy_a 50", "imu_dt 0.0025"):  # (the other value of each pair is taken)
            SINGLE[name](p)


SINGLE = {
    "surfel_sigma0 0.05": _set("surfel_sigma0", 0.05),
    "surfel_sigma0 1e-3": _set("surfel_sigma0", 1e-3),
    "cauchy_a 0.05": _set("cauchy_a", 0.05),
    "cauchy_a 50": _set("cauchy_a", 50.0),
    "imu_dt 0.0025": _set("imu_dt", 0.0025),
    "imu_dt 0.01": _set("imu_dt", 0.01),
    "w_gyr x 3": _scale("w_gyr", 3.0),
    "w_acc / 3": _scale("w_acc", 1.0 / 3.0),
    "w_bg x 3": _scale("w_bg", 3.0),
    "w_ba / 3": _scale("w_ba", 1.0 / 3.0),
}
CASES = dict(SINGLE)
CASES["everything together"] = _all  # surfel_sigma0 0.05, cauchy_a 0.05, imu_dt 0.01, w_gyr x 3, w_acc / 3, w_bg x 3, w_ba / 3

_SURFEL = ((ROT, ROT), (ROT, POS), (POS, POS))
REACH = {
    "surfel_sigma0 0.05": _SURFEL, "surfel_sigma0 1e-3": _SURFEL, "cauchy_a 0.05": _SURFEL, "cauchy_a 50": _SURFEL,
    # 1 / dt scales the gyroscope rows' rot columns (their b1 columns are the weight alone), 1 / dt^2 the accelerometer rows' pos columns
    "imu_dt 0.0025": ((ROT, ROT), (ROT, B1), (POS, POS), (POS, B2)), "imu_dt 0.01": ((ROT, ROT), (ROT, B1), (POS, POS), (POS, B2)),
    "w_gyr x 3": ((ROT, B1), (B1, B1)),
    "w_acc / 3": ((POS, B2), (ROT, B2), (B2, B2)),
    "w_bg x 3": ((B1, B1),),
    "w_ba / 3": ((B2, B2),),
    "everything together": _SURFEL + ((ROT, B1), (B1, B1), (POS, B2), (B2, B2)),
}
WINDOWS = ("default ns=8", "six modes quirks=1", "six modes quirks=0")
SOLVE_CASES = ("everything together", "cauchy_a 0.05")


def case_params(oracle, name, base=None):
    """oracle.default_params() (or a copy of base's switches: reference_quirks, max_iterations) with the case applied"""
    p = oracle.default_params()
    if base is not None:
        p.reference_quirks, p.max_iterations = base.reference_quirks, base.max_iterations
    if name is not None:
        CASES[name](p)
    return p


_CACHE = {}


def window(oracle, which):
    """the spec (tests/linearize_ref.py) of one of WINDOWS under the default parameters: the default family at 8 sample states (IMU
    factors, the gauge held) and the six-mode window of test_linearize_gpu.py::test_all_six_factor_modes_with_and_without_quirks.
    Built once; with_case() derives the cases from it"""
    if which not in _CACHE:
        if which == "default ns=8":
            sp = lr.from_problem(lr.window_problem(oracle, 8))
        else:
            from test_window_gpu import _mode2_pairs
            from wildcat_slam_amd import synth

            w = synth.surfel_window(3, 300, seed=11, fixed_patches=120, sample_dt=0.08)
            params = oracle.default_params()
            params.reference_quirks = 1 if which.endswith("=1") else 0
            pairs = np.concatenate([oracle.match(w["surf"], w["pose"], w["surf"], w["pose"], True, params), _mode2_pairs(w, 25, np.random.default_rng(11))])
            pf = oracle.match(w["surf"], w["pose"], w["fix_surf"], w["fix_pose"], False, params)
            sp = lr.spec(w, params, pairs, pf, True, w["imu"])
        _CACHE[which] = sp
    return _CACHE[which]


def with_case(oracle, sp, name):
    """the same window - same surfels, poses, correspondences, IMU states, gauge - under the case's parameters (None: the default's)"""
    out = dict(sp)
    out["params"] = case_params(oracle, name, base=sp["params"])
    return out


def points(sp, seed=7):
    ns = len(sp["w"]["sample_times"])
    return np.zeros(12 * ns), lr.random_point(ns, seed)


def excess(e, floor, allow):
    """a result's errors over check_linearization's bars: (4 x 4 ratios of eH by type pair, eg ratio, cost ratio)"""
    bH, bg, bc = lr.bars(floor, allow)
    return e["eH_types"] / bH, e["eg"] / bg, e["ec"] / bc


def raw_r2(res_surfel, cauchy_a):
    """r^2 of the surfel factors from their loss-corrected residuals r_c = r / sqrt(1 + r^2 / b), b = cauchy_a^2: r^2 = q / (1 - q / b),
    q = r_c^2 (q < b always; r^2 > b exactly when q > b / 2)"""
    b = cauchy_a * cauchy_a
    q = np.asarray(res_surfel, np.float64) ** 2
    return q / np.maximum(1.0 - q / b, np.finfo(np.float64).tiny)
