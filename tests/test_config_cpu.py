"""The facade's configuration on the CPU: what LidarOdometry derives from a LioConfig (host/lidar_odometry.cc: WcParamsFromConfig, through
wc_host_params_from_config - no context, no GPU) and what the orchestrated oracle derives from the same values (oracle/odometry.cc:
derive, its own statement of lio_config.h:42-45), each against the Python float evaluation of the reference's expressions; the byte
equality of the default configuration's wc_params with wc_params_default; and the proof that the two configurations of
tests/test_facade_gpu.py::test_facade_non_default_configuration_against_the_oracle are live.

Bit for bit: 1 / (n * sqrt(rate)) * k and 1 / (w / sqrt(rate)) * k are chains of correctly rounded IEEE operations (sqrt, *, /) in
Python as in C++; both libraries are built with -ffp-contract=off and the expressions hold no a * b + c to contract anyway, so no ulp
is allowed."""
import math

import numpy as np
import pytest

import config_cases as cc
from wildcat_slam_amd import lib

D = cc.D
CASES = {
    "default": {},
    "gyroscope_noise_density x 2": dict(gyroscope_noise_density=2 * D["gn"]),
    "accelerometer_noise_density x 2": dict(accelerometer_noise_density=2 * D["an"]),
    "gyroscope_random_walk x 2": dict(gyroscope_random_walk=2 * D["gw"]),
    "accelerometer_random_walk x 2": dict(accelerometer_random_walk=2 * D["aw"]),
    "imu_factor_weight 0.03": dict(imu_factor_weight=0.03),
    "imu_rate 100": dict(imu_rate=100.0),
    "imu_rate 400": dict(imu_rate=400.0),
    "all of the IMU model": dict(gyroscope_noise_density=3.1e-4, accelerometer_noise_density=7.7e-3, gyroscope_random_walk=9.3e-5,
                                 accelerometer_random_walk=4.1e-6, imu_factor_weight=0.07, imu_rate=125.0),
}


def _expected(fields):
    """lio_config.h:42-45 in Python floats"""
    c = lib.default_config().update(**fields)
    rate, k = c.imu_rate, c.imu_factor_weight
    return dict(w_gyr=1 / (c.gyroscope_noise_density * math.sqrt(rate)) * k, w_acc=1 / (c.accelerometer_noise_density * math.sqrt(rate)) * k,
                w_bg=1 / (c.gyroscope_random_walk / math.sqrt(rate)) * k, w_ba=1 / (c.accelerometer_random_walk / math.sqrt(rate)) * k,
                imu_dt=1 / rate)


def test_default_config_gives_the_bytes_of_wc_params_default(oracle):
    p, rc = lib.host_params_from_config(None)
    assert rc == lib.WC_OK and bytes(p) == bytes(lib.default_params())
    p, rc = lib.host_params_from_config(lib.default_config())
    assert rc == lib.WC_OK and bytes(p) == bytes(lib.default_params())
    o = oracle.Odometry()
    assert bytes(o.params()) == bytes(oracle.default_params()) == bytes(lib.default_params())
    assert o.config() == lib.default_config().to_dict()  # the two sides start from the same configuration values
    o.close()


@pytest.mark.parametrize("name", list(CASES))
def test_cost_weights_follow_the_configuration_on_both_sides(oracle, name):
    fields, want = CASES[name], _expected(CASES[name])
    p, rc = lib.host_params_from_config(lib.default_config().update(**fields))
    assert rc == lib.WC_OK
    o = oracle.Odometry()
    o.set_config(**fields)
    q = o.params()
    for k, v in want.items():
        assert getattr(p, k) == v, ("facade", name, k, getattr(p, k), v)
        assert getattr(q, k) == v, ("oracle", name, k, getattr(q, k), v)
    assert bytes(p) == bytes(q)
    # what the configuration does not reach is wc_params_default's
    d = lib.default_params()
    for k, _ in lib.R.Params._fields_:
        if k not in want and k != "view_point":
            assert getattr(p, k) == getattr(d, k), k
    # ... and a field that changed moved the weight it belongs to, and only that one
    moved = set(k for k in want if getattr(p, k) != getattr(d, k))
    expect_moved = {"default": set(), "gyroscope_noise_density x 2": {"w_gyr"}, "accelerometer_noise_density x 2": {"w_acc"},
                    "gyroscope_random_walk x 2": {"w_bg"}, "accelerometer_random_walk x 2": {"w_ba"},
                    "imu_factor_weight 0.03": {"w_gyr", "w_acc", "w_bg", "w_ba"}}.get(name, set(want))
    assert moved == expect_moved, (name, moved)
    o.close()


def test_iteration_limit_and_refusals_without_a_context():
    p, rc = lib.host_params_from_config(lib.default_config().update(inner_iter_num_max=7))
    assert rc == lib.WC_OK and p.max_iterations == 7
    # a configuration whose derived parameters wc_params_check refuses: a zero noise density is an infinite weight, imu_rate = 0 an
    # infinite imu_dt, a negative iteration limit
    for fields in (dict(gyroscope_noise_density=0.0), dict(accelerometer_random_walk=0.0), dict(imu_rate=0.0), dict(imu_rate=float("nan")),
                   dict(imu_factor_weight=float("inf")), dict(imu_factor_weight=-0.01), dict(inner_iter_num_max=-1)):
        p, rc = lib.host_params_from_config(lib.default_config().update(**fields))
        assert rc == lib.WC_ERR_ARG and lib.params_check(p)[0] == lib.WC_ERR_ARG, fields
    with pytest.raises(TypeError):
        lib.default_config().update(no_such_field=1.0)


def _run(oracle, msgs, imu, fields):
    o = oracle.Odometry()
    o.set_config(**fields)
    rec = []
    cc.feed(o, msgs, imu, lambda k: rec.append((o.samples().copy(), dict(o.stats()))))
    o.close()
    return rec


def _differs(a, b):
    """does a sweep of one run differ from the other's by more than the bars of the facade's per-sweep comparison: another number of
    sample states, surfels or correspondences (exact there, or within 2), or sample states further apart than its 1e-6"""
    (sa, ta), (sb, tb) = a, b
    if sa.shape != sb.shape or any(ta[k] != tb[k] for k in ("sld_surfels", "fix_surfels")) or any(abs(ta[k] - tb[k]) > 2 for k in ("binary", "unary")):
        return True
    from test_facade_gpu import _state_diff

    return _state_diff(sa, sb) > 1e-6


@pytest.mark.parametrize("name", list(cc.CONFIGS))
def test_each_facade_configuration_is_live(oracle, name):
    """the oracle under the default configuration against the oracle under the test configuration on the test's stream: a facade that
    ignored the configuration would be the former.  Measured: imu_model - sample states 0.20, 0.78 and 0.91 apart in sweeps 1 to 3;
    timing_preprocessing_extrinsics - 7 / 13 sample states against 5 / 9 / 13 and two sweeps completed against three."""
    msgs, imu, _ = cc.stream(name)
    test = _run(oracle, msgs, imu, cc.CONFIGS[name]["config"])
    assert len(test) == cc.SWEEPS  # the shortest stream that completes three sweeps ...
    assert len(_run(oracle, msgs[:-1], imu, cc.CONFIGS[name]["config"])) < cc.SWEEPS  # ... one message less does not
    default = _run(oracle, msgs, imu, {})
    assert len(default) != len(test) or any(_differs(a, b) for a, b in zip(default, test)), name
    if name == "imu_model":
        # ... and with imu_rate taken but the noise densities and imu_factor_weight ignored (the facade read neither before it formed
        # the weights from them): every sweep differs.  Measured: sample states 2.4e-3, 6.4e-3 and 6.9e-3 apart
        rate_only = _run(oracle, msgs, imu, dict(imu_rate=100.0))
        assert len(rate_only) == len(test) and all(_differs(a, b) for a, b in zip(rate_only, test))
