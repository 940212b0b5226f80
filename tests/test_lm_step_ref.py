"""The reference of tests/test_lm_step_gpu.py checked on the CPU: the Dot2 residual against exact rational arithmetic, the refined
solve against its own residual, and the restated LM step (scaling, clamp of the diagonal, damping, gauge rows) against the
oracle's first step (oracle/window.cc), the solve the rest of the suite trusts."""
from fractions import Fraction

import numpy as np
import pytest

import lm_step_ref as ref


def test_dot2_residual_is_exact_to_one_rounding():
    """r = A y - b by Dot2 equals the exact rational residual rounded once (within one unit in its last place), also where the
    residual is a billionth of the terms it is made of and where the terms span sixteen decades"""
    rng = np.random.default_rng(0)
    for t in range(60):
        n = int(rng.integers(2, 10))
        A = rng.normal(size=(n, n)) * 10.0 ** rng.integers(-8, 9, size=(n, n))
        y = rng.normal(size=n)
        b = (A @ y) * (1.0 + 10.0 ** -rng.integers(6, 10) * rng.normal(size=n))
        r = ref.dot2_residual(A, y, b)
        exact = [sum((Fraction(A[i, j]) * Fraction(y[j]) for j in range(n)), Fraction(0)) - Fraction(b[i]) for i in range(n)]
        rounded = np.array([float(e) for e in exact])
        assert np.all(np.abs(r - rounded) <= np.spacing(np.abs(rounded))), (t, r, rounded)
    # what plain float64 loses here, Dot2 keeps: sum of 1e16, 1, -1e16 (exactly 1)
    A = np.array([[1e16, 1.0, -1e16]])
    assert ref.dot2_residual(A, np.ones(3), np.zeros(1))[0] == 1.0
    assert (A @ np.ones(3))[0] != 1.0


def test_refined_solve_has_a_residual_at_rounding_level():
    rng = np.random.default_rng(1)
    n = 60
    Q = np.linalg.qr(rng.normal(size=(n, n)))[0]
    A = (Q * np.logspace(0, -10, n)) @ Q.T  # SPD, condition number 1e10
    A = 0.5 * (A + A.T)
    b = rng.normal(size=n)
    y = ref.solve(A, b)
    assert ref.backward_errors(A, b, y)["all"] <= 1e-16
    assert ref.backward_errors(A, b, np.linalg.solve(A, b))["all"] <= 1e-13  # (the measure itself: an unrefined solve passes too)
    A2 = (Q * np.logspace(0, -1, n)) @ Q.T  # (the measure is normwise: an error shows in proportion to ||A|| ||y||)
    y2 = ref.solve(A2, b)
    assert ref.backward_errors(A2, b, y2)["all"] <= 1e-16
    assert ref.backward_errors(A2, b, y2 * (1 + 1e-9))["all"] > 1e-11  # ... and a solution wrong by 1e-9 does not


@pytest.mark.parametrize("ns,fix_first,with_imu", [(6, True, True), (6, False, True), (9, True, False), (9, False, False),
                                                   (20, True, True), (20, False, True)])
def test_reference_step_is_the_oracles_first_step(oracle, ns, fix_first, with_imu):
    """oracle.Window.solve with max_iterations = 1 keeps only the unknowns the gauge leaves (window.cc: `act`); the reference keeps
    all 12 ns, the gauge rows as zero rows of H and g.  Same step to 1e-12 relative, and the gauge rows' step is exactly zero."""
    prob = ref.window_problem(oracle, ns, "default" if fix_first else "free_gauge", seed=5)
    if not with_imu:
        prob["imu"] = None
    W = ref.oracle_window(oracle, prob)
    x0 = np.zeros(12 * ns)
    H, g, _ = W.linearize(x0)
    _, s, first = W.solve(x0)
    assert s.iterations == 1 and s.first_step[0] > 0
    step = ref.reference_step(H, g)
    assert np.abs(step - first).max() <= 1e-12 * np.abs(first).max(), np.abs(step - first).max() / np.abs(first).max()
    assert abs(np.linalg.norm(step) - s.first_step[0]) <= 1e-12 * s.first_step[0]
    if fix_first:
        assert not H[3:6].any() and not step[3:6].any() and not first[3:6].any()
    A, gs, scale = ref.damped_system(H, g, 1e4)
    eta = ref.backward_errors(A, gs, -step / scale, ref.pose_bias_rows(ns))
    assert max(eta.values()) <= 1e-16, eta


def test_weak_imu_family_clamps_bias_unknowns(oracle):
    """the weak_imu family of the GPU test reaches the LM clamp of the diagonal (diag(S H S) < 1e-6) on real bias unknowns"""
    prob = ref.window_problem(oracle, 9, "weak_imu")
    H, g, _ = ref.oracle_window(oracle, prob).linearize(np.zeros(12 * 9))
    d = np.diag(H) / (1.0 + np.sqrt(np.diag(H))) ** 2
    bias = ref.pose_bias_rows(9)["bias"]
    assert np.count_nonzero(d[bias] < 1e-6) >= 9 * 3
