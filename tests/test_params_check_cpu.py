"""wc_params_check (csrc/ctx.hip), the host-side gate wc_ctx_create and wc_ctx_set_params go through: no context, no GPU.  Per field the
values that must be refused - each would put a NaN or an infinity into a kernel (1 / imu_dt in the IMU Jacobians, 1 / cauchy_a^2 in the
loss, 1 / surfel_sigma0 in the surfel weight, the matcher's features divided by center_scale and angular_scale before the kd-tree is
built, the voxel index of a point) - and the edge that must stay accepted: the smallest positive double or float, the largest finite
one, and every value the suite's other tests set (a negative angular_scale, angular_scale = 3.2, surfel_dist_max = 1e3, time_diff_min = 0,
IMU weights x 1e-6, cluster_gap = 2e-4, voxel sizes 0.125 to 0.95).  The name returned is the field's."""
import copy
import ctypes as C

import numpy as np
import pytest

from wildcat_slam_amd import lib

NAN, INF = float("nan"), float("inf")
TINY, HUGE = 5e-324, 1.7976931348623157e308  # the smallest positive (subnormal) and the largest finite double
FTINY, FHUGE = float(np.float32(1e-45)), float(np.finfo(np.float32).max)  # ... and float (voxel_size and planer_threshold are floats)
I32 = 2 ** 31 - 1

FINITE_POS = (NAN, INF, -INF, 0.0, -0.0, -1.0, -TINY)
FINITE_NONNEG = (NAN, INF, -INF, -1.0, -TINY)
FINITE = (NAN, INF, -INF)
FINITE_NONZERO = (NAN, INF, -INF, 0.0, -0.0)
NOT_NAN = (NAN,)

# field: (refused values, accepted values)
RULES = {
    "voxel_size": ((NAN, INF, -INF, 0.0, -0.0, -1.0, -FTINY), (FTINY, FHUGE, 0.125, 0.8, 0.95)),
    "max_layer": ((-1, 3, I32, -I32 - 1), (0, 1, 2)),
    "min_points": ((-1, -I32 - 1), (0, 20, I32)),
    "planer_threshold": ((NAN, INF, -INF, -1.0, -FTINY), (0.0, FTINY, FHUGE, 0.01)),
    "min_plane_likeness": (FINITE, (0.0, -HUGE, HUGE, 0.1, -1.0)),
    "cluster_gap": (FINITE_NONNEG, (0.0, TINY, HUGE, 2e-4, 0.05)),
    "cluster_min_points": ((0, -1, -I32 - 1), (1, 20, I32)),
    "center_scale": (FINITE_NONZERO, (TINY, -TINY, HUGE, -HUGE, 1.0, 0.1, 10.0)),
    "angular_scale": (FINITE_NONZERO, (TINY, -TINY, HUGE, -HUGE, 3.2, -5.0 * np.pi / 180.0, np.pi / 180.0)),
    "surfel_dist_max": (NOT_NAN, (INF, -INF, 0.0, -1.0, 1e3, 0.1, HUGE)),
    "knn_k": ((0, -1, 17, I32), (1, 10, 16)),
    "time_diff_min": (NOT_NAN, (INF, -INF, 0.0, -1.0, 0.06, 1.0)),
    "surfel_sigma0": (FINITE_POS, (TINY, HUGE, 1e-3, 0.05)),
    "cauchy_a": (FINITE_POS, (TINY, HUGE, 0.05, 50.0)),
    "w_gyr": (FINITE_NONNEG, (0.0, TINY, HUGE, 4.65e-5)),
    "w_acc": (FINITE_NONNEG, (0.0, TINY, HUGE, 1.12e-6)),
    "w_bg": (FINITE_NONNEG, (0.0, TINY, HUGE, 1.2e-3)),
    "w_ba": (FINITE_NONNEG, (0.0, TINY, HUGE, 5.3e-2)),
    "imu_dt": (FINITE_POS, (TINY, HUGE, 0.0025, 0.01)),
    "max_iterations": ((-1, -I32 - 1), (0, 1, 100, I32)),
}


def _with(field, value):
    p = lib.default_params()
    setattr(p, field, value)
    return p


def test_the_defaults_pass_and_every_field_has_a_rule(oracle):
    assert lib.params_check(lib.default_params()) == (lib.WC_OK, None)
    assert lib.params_check(oracle.default_params()) == (lib.WC_OK, None)
    # reference_quirks and exact_sums are switches (any value is one of two behaviours); every other field is in the table
    fields = [name for name, _ in lib.R.Params._fields_]
    assert set(fields) - set(RULES) == {"view_point", "reference_quirks", "exact_sums"}
    assert lib.load().wc_params_check(C.byref(lib.default_params()), None) == lib.WC_OK  # (the field pointer may be NULL)
    assert lib.load().wc_params_check(None, None) == lib.WC_ERR_ARG


@pytest.mark.parametrize("field", sorted(RULES))
def test_refused_and_accepted_values(field):
    refused, accepted = RULES[field]
    for v in refused:
        assert lib.params_check(_with(field, v)) == (lib.WC_ERR_ARG, field), (field, v)
    for v in accepted:
        assert lib.params_check(_with(field, v)) == (lib.WC_OK, None), (field, v)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_view_point_must_be_finite(axis):
    for v, want in ((NAN, lib.WC_ERR_ARG), (INF, lib.WC_ERR_ARG), (-INF, lib.WC_ERR_ARG), (HUGE, lib.WC_OK), (-HUGE, lib.WC_OK), (3.5, lib.WC_OK)):
        p = lib.default_params()
        p.view_point[axis] = v
        assert lib.params_check(p) == (want, "view_point" if want else None), (axis, v)


def test_values_the_other_tests_set_stay_accepted():
    """together, as tests/lm_step_ref.py (weak_imu), tests/match_gates.py and tests/test_match_gpu.py set them"""
    p = lib.default_params()
    for k in ("w_gyr", "w_acc", "w_bg", "w_ba"):
        setattr(p, k, getattr(p, k) * 1e-6)
    p.angular_scale, p.surfel_dist_max, p.time_diff_min, p.cluster_gap, p.voxel_size = -p.angular_scale, 1e3, 0.0, 2e-4, 0.125
    assert lib.params_check(p) == (lib.WC_OK, None)


def test_the_first_refused_field_in_declaration_order_is_named():
    p = lib.default_params()
    p.imu_dt, p.cauchy_a = 0.0, NAN
    assert lib.params_check(p) == (lib.WC_ERR_ARG, "cauchy_a")
    p.center_scale = 0.0
    assert lib.params_check(p) == (lib.WC_ERR_ARG, "center_scale")


def test_create_refuses_before_it_looks_for_a_device():
    """wc_ctx_create with refused parameters is WC_ERR_ARG whether or not a GPU is there: nothing of the device is touched for them"""
    h = C.c_void_p(0)
    bad = _with("imu_dt", 0.0)
    assert lib.load().wc_ctx_create(C.byref(bad), C.c_int(0), C.byref(h)) == lib.WC_ERR_ARG and not h.value
    untouched = copy.copy(bytes(bad))
    assert lib.params_check(bad)[0] == lib.WC_ERR_ARG and bytes(bad) == untouched  # (the check writes nothing into the parameters)
