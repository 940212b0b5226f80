"""The damped LM step of the window solve, kernel level: the step the GPU took (wc_window_solve's first increment, max_iterations = 1)
against the damped system built from the GPU's OWN H and g (tests/lm_step_ref.py), so that assembly errors drop out and the bar can
sit near rounding level.  Measure: the normwise backward error of y = -step / scale,
    eta = ||A y - gs||_inf / (||A||_inf ||y||_inf + ||gs||_inf)        (residual by Dot2: twice the working precision)
over all rows and, with each row block's own norms, over the pose rows and over the bias rows alone (an error confined to the bias
unknowns does not hide behind the pose rows).  A structural defect - a skipped tile or column chunk, a wrong reduction level, the
damping on the wrong entries, a lost coupling block - gives 1e-8 or more; rounding gives 1e-16 to 1e-13.

Both forms at every size the window build accepts a boundary of: the default (bias elimination by parallel cyclic reduction, then
the dense panel steps on the pose half; ns < 4 take the dense path; above a radius of 10^lm_dense_radius = 1e7 the dense step) and
lm_dense = 1.  The default form's step must be its own: a dense re-try of a rejected or invalid step (summary.first_step[1]) would
hide a broken elimination behind the dense step.

Bars.  The dense form, and the default form at radius <= 1e4 and above the switch (where it is the dense step): 1e-12.  The
elimination at its largest radius, 1e7: 1e-12 for the no_imu and weak_imu families, 1e-9 for default, free_gauge and one_plane.
The elimination inverts 12 x 12 blocks explicitly and does not pivot; its backward error in the bias rows is about cond(T) eps, and
cond(T) of the damped bias block grows with the radius (2e4 at 1e4, 2e9 at 1e9 for ns = 33), while the dense form meets 1e-15 on
the same systems: the known conditioning limit of PCR without pivoting.  It set the switch: the largest radius at which the
elimination stays below 1e-9 is 1e7 (forced at 4 to 340 sample states over the five families: at most 1.9e-10 at 1e7, 1.4e-9 at
1e8, 1.2e-8 at 1e9).  Above the switch the elimination (lm_dense_radius = 0) is measured and printed, not asserted.

Measured worst eta on the MI355X (all rows / pose rows / bias rows; the table a run with -s prints at the end):
    dense form, every radius and family                 1.1e-15 / 9.8e-16 / 1.6e-15
    elimination, radius <= 1e4, every family            1.1e-15 / 1.1e-15 / 1.1e-15
    elimination, radius 1e7, default / one_plane        5.7e-11 / 3.9e-16 / 1.1e-10
    elimination, radius 1e7, free_gauge                 7.0e-11 / 3.3e-16 / 1.5e-10
    elimination, radius 1e7, no_imu / weak_imu          2.2e-16 / 2.2e-16 / 6.7e-14
    elimination forced, radius 1e9 (printed)            4.3e-09 / 2.2e-14 / 1.2e-08
    elimination forced, radius 1e12 (printed)           8.9e-08 / 1.1e-12 / 2.5e-07"""
import math

import numpy as np
import pytest

import lm_step_ref as ref

pytestmark = pytest.mark.gpu

# every boundary of the step's shape logic: PCR levels ceil(log2((ns + 1) / 2)) change at 9, 17, 33, 65, 129, 257; odd ns adds a
# phantom identity super-block; column chunks ceil(roundup(6 ns + 1, 64) / 256) change at 43, 86, 128, 171, 214, 256, 299; the
# buffers are sized by max(ns, 96); ns = 2, 3 take the dense path; 340 is the largest window the build accepts
NS = (2, 3, 4, 5, 8, 9, 16, 17, 33, 42, 43, 64, 65, 85, 86, 96, 97, 127, 128, 129, 130, 170, 171, 213, 214, 255, 256, 257, 298, 299,
      339, 340)
RADII_NS = (2, 5, 9, 33, 86, 129, 256, 340)  # where the step is also taken at radius 1e-2, 1e7, 1e9 and 1e12
RADII = (1e-2, 1e4, 1e7, 1e9, 1e12)
FAMILY_NS = (5, 65, 171, 340)
SWITCH = 1e7  # 10^lm_dense_radius (the library's default, 7): above it the default form takes the dense step
DEFAULTS = {"lm_dense": 0, "lm_radius0": -1, "lm_dense_radius": 7}
BOUND = 1e-12
PCR_BOUND = {"default": 1e-9, "free_gauge": 1e-9, "one_plane": 1e-9, "no_imu": BOUND, "weak_imu": BOUND}  # elimination, 1e4 < radius <= SWITCH
ETAS = []


@pytest.fixture(scope="module")
def ctx():
    """a context of its own: the step is taken with max_iterations = 1 and window-specific parameters"""
    from wildcat_slam_amd import lib

    c = lib.Context(0)
    yield c
    if ETAS:
        print("\nworst eta (all / pose / bias) by form and family:")
        for key in sorted({(e[0], e[1], e[2]) for e in ETAS}):
            rows = [e[3] for e in ETAS if (e[0], e[1], e[2]) == key]
            print("  %-12s %-10s %-13s %s" % (key + (" / ".join("%.1e" % max(r[k] for r in rows) for k in ("all", "pose", "bias")),)))
    c.close()


def _build(ctx, oracle, ns, family="default", seed=11):
    prob = ref.window_problem(oracle, ns, family, seed)
    w = prob["w"]
    ctx.set_params(prob["params"])
    keep = [ctx.to_device(a) for a in (w["surf"], w["pose"], prob["pairs"], w["fix_surf"], w["fix_pose"], prob["pf"])]
    ctx.window_build(keep[0], keep[1], keep[2], len(prob["pairs"]), prob["imu"], w["sample_times"], w["grav"], prob["fix_first"], keep[3],
                     keep[4], keep[5], len(prob["pf"]))
    H, g, _ = ctx.window_linearize(np.zeros(12 * ns))
    return keep, H, g


def _first_step(ctx, n, radius, **opts):
    if radius != 1e4:
        opts["lm_radius0"] = int(round(math.log10(radius)))
    try:
        for k, v in opts.items():
            ctx.set_dev_option(k, v)
        _, s, first = ctx.window_solve(np.zeros(n))
    finally:
        for k, v in DEFAULTS.items():
            ctx.set_dev_option(k, v)
    return s, first


def _eta(system, s, first, tag):
    A, gs, scale = system
    assert s.iterations == 1 and s.first_step[0] > 0, tag  # (a step was taken at this radius: the first attempt was valid)
    assert np.all(np.isfinite(first)), tag
    assert abs(np.linalg.norm(first) - s.first_step[0]) <= 1e-12 * s.first_step[0], tag
    eta = ref.backward_errors(A, gs, -first / scale, ref.pose_bias_rows(len(gs) // 12))
    print("eta %-44s all %.2e  pose %.2e  bias %.2e  retries %d" % (tag, eta["all"], eta["pose"], eta["bias"], s.first_step[1]))
    return eta


def _check_window(ctx, oracle, ns, family, radii):
    keep, H, g = _build(ctx, oracle, ns, family)
    n = 12 * ns
    for radius in radii:
        system = ref.damped_system(H, g, radius)
        tag = "ns=%d %s r=%.0e" % (ns, family, radius)
        sd, fd = _first_step(ctx, n, radius, lm_dense=1)
        eta = _eta(system, sd, fd, tag + " dense")
        ETAS.append(("dense", "every", "every radius", eta))
        assert max(eta.values()) <= BOUND, (tag, "dense", eta)
        s, first = _first_step(ctx, n, radius)
        elim = ns >= 4 and radius <= SWITCH  # (what the library takes with its defaults)
        eta = _eta(system, s, first, tag + (" elimination" if elim else " default (dense)"))
        # the reported step is the form's own, not a dense re-try; a correct step can be rejected (rho <= 1e-3) - then the dense form
        # rejects it too, and the case wants another seed
        assert s.first_step[1] == 0, (tag, "dense re-try", "the dense form %s its first step" % ("rejects" if sd.unsuccessful_steps else "accepts"))
        if elim and radius > 1e4:
            ETAS.append(("elimination", family, "r=1e7", eta))
            assert max(eta.values()) <= PCR_BOUND[family], (tag, "elimination", eta)
        else:
            ETAS.append(("elimination" if elim else "dense", family if elim else "every", "r<=1e4" if elim else "every radius", eta))
            assert max(eta.values()) <= BOUND, (tag, eta)
        if ns >= 4 and radius > SWITCH:  # the elimination forced above the switch: measured and printed, not asserted
            s, first = _first_step(ctx, n, radius, lm_dense_radius=0)
            if s.first_step[1] == 0:
                ETAS.append(("forced", "every", "r=%.0e" % radius, _eta(system, s, first, tag + " elimination forced")))
            else:  # (rejected and taken again densely: the reported step is not the elimination's)
                print("eta %-44s re-tried densely" % (tag + " elimination forced"))
    return H, g, keep


@pytest.mark.parametrize("ns", NS)
def test_lm_step_backward_error(ctx, oracle, ns):
    """the default window (gauge held, IMU factors) at every boundary size: radius 1e4 (the solve's first step), and at RADII_NS
    also 1e-2 (the damping dominates: a misplaced damping term shows at once), 1e7 (the elimination's largest radius), 1e9 and 1e12
    (the dense step by the lm_dense_radius switch; with lm_dense_radius = 0 the elimination, printed)"""
    _check_window(ctx, oracle, ns, "default", RADII if ns in RADII_NS else (1e4,))


@pytest.mark.parametrize("family", ref.FAMILIES[1:])
@pytest.mark.parametrize("ns", FAMILY_NS)
def test_lm_step_backward_error_families(ctx, oracle, ns, family):
    """free_gauge (fix_first_pos = 0, the gauge held by the IMU factors), no_imu (the bias block is damping only), one_plane
    (lidar leaves two translations and yaw unobservable), weak_imu (bias unknowns under the clamp of the diagonal)"""
    H, g, _ = _check_window(ctx, oracle, ns, family, RADII)
    if family == "weak_imu":  # the family tests the clamp: real bias unknowns (not the gauge's) have diag(S H S) below 1e-6
        d = np.diag(H) / (1.0 + np.sqrt(np.diag(H))) ** 2
        bias = ref.pose_bias_rows(ns)["bias"]
        assert np.count_nonzero(d[bias] < 1e-6) >= ns
