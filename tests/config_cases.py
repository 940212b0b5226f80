"""The two non-default facade configurations of tests/test_facade_gpu.py::test_facade_non_default_configuration_against_the_oracle and
of the CPU half in tests/test_config_cpu.py (which shows that each is live: the oracle under the default configuration differs from
the oracle under the test configuration by more than the GPU test's bars), and the streams they run on: the shortest that completes
three sweeps."""
import numpy as np

D = dict(gn=0.00015198973532354657, an=0.006308226052016165, gw=0.00011673723527962174, aw=2.664506559330434e-06)  # lio_config.h:10-13


def _rot(axis, angle):
    """Rodrigues' rotation matrix"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


EXT_R0 = np.array([[-5.32125e-08, -1, 0], [-1, -5.32125e-08, -0], [0, 0, -1]])  # lio_config.h:25-28

CONFIGS = {
    # the IMU model: both noise densities x 2, another weight between IMU and lidar factors, a 100 Hz IMU (imu_dt = 0.01 and sqrt(100) in
    # every cost weight)
    "imu_model": dict(
        config=dict(gyroscope_noise_density=2 * D["gn"], accelerometer_noise_density=2 * D["an"], imu_factor_weight=0.03, imu_rate=100.0),
        stream=dict(duration=1.5, pts_per_s=300_000, gyro_bias=(0.0, 0.0, 0.02), t_start=1000.0, imu_rate=100.0)),
    # timing, preprocessing and extrinsics: another sample-state spacing and sweep length, gravity, range gate, a shifted blind box, the
    # lidar mounted 5 cm / 3 cm / 2 cm elsewhere and turned by 2 degrees
    "timing_preprocessing_extrinsics": dict(
        config=dict(sample_dt=0.1, sweep_duration=0.4, gravity_norm=9.80, min_range=1.0, max_range=30.0,
                    blind_min=(-0.6, -0.7, -0.4), blind_max=(0.5, 0.3, 0.4), ext_translation=(0.049, -0.03855, 0.075),
                    ext_rotation=(_rot((1.0, 2.0, 3.0), np.deg2rad(2.0)) @ EXT_R0).reshape(-1).tolist()),
        stream=dict(duration=1.3, pts_per_s=300_000, gyro_bias=(0.0, 0.0, 0.02), t_start=1000.0)),
}
SWEEPS = 3


def stream(name):
    from wildcat_slam_amd import synth

    kw = dict(CONFIGS[name]["stream"])
    return synth.raw_stream(kw.pop("duration"), **kw)


def feed(odo, msgs, imu, on_sweep=None):
    """the raw stream into one odometry (the facade or the orchestrated oracle); on_sweep(sweep number) after every completed sweep"""
    k = 0
    for m in msgs:
        if len(m) == 0:
            continue
        while k < len(imu["t"]) and imu["t"][k] <= m["time"][-1] + 0.02:
            odo.add_imu(imu["t"][k], imu["acc"][k], imu["gyr"][k])
            k += 1
        before = odo.sweeps()
        odo.add_scan(m)
        if on_sweep is not None and odo.sweeps() != before:
            on_sweep(odo.sweeps())
