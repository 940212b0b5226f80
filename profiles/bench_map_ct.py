"""Timings of the continuous-time registration against the voxel map (csrc/map.hip: k_map_linearize_ct, k_map_lin_reduce<80, 76>;
include/wildcat_hip.h "registration of a stamped sweep in continuous time") beside the rigid registration it extends, in one process, on
the 11-sweep map of bench_map_surfels.py (1 M-point sweeps of the room of synth.g1_room, v = 0.05 and 0.2).  Prints ONE JSON object and
writes it to profiles/map_ct_bench.json:
  linearize_ms       wc_map_linearize of 1 M points at the identity pose, the Cauchy loss on (a = 0.4), no d_rows: the yardstick
  linearize_ct_ms    wc_map_linearize_ct of the same 1 M points with their stamps, both poses the identity, without and with d_xyz_out:
                     the same search, 8 (20) more bytes per point, 76 sums instead of 28; reduction launches and the 640-byte read-back
                     inside the timed span
  align_ct           one wc_map_align_ct of the query sweep measured again from a sensor that moves 5 cm and 1 degree, from starts 2 cm
                     and 3 mrad off: wall and device time of the whole loop, iterations, termination and the pose errors left
Every device figure: median and minimum of --reps device-timed calls (wc_timer_start / wc_timer_stop_ms) after 3 warm-up calls.
python profiles/bench_map_ct.py [--reps 20] [--out profiles/map_ct_bench.json]"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "wildcat-slam_amd", "python"))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import numpy as np  # noqa: E402

import map_ct_ref as CT  # noqa: E402  (the sweep simulator and the pose helpers)
from map_bench_common import timed, xyz_of  # noqa: E402
from wildcat_slam_amd import lib, synth  # noqa: E402
from wildcat_slam_amd import records as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(HERE, "map_ct_bench.json"))
    a = ap.parse_args()
    reps = max(3, a.reps)
    ctx = lib.Context(0)
    n_sweep = 1_000_000
    sweeps = [synth.g1_room(n_sweep, seed=200 + i, t_start=1000.0 + 0.5 * i) for i in range(11)]
    query = synth.g1_room(n_sweep, seed=300, t_start=2000.0)
    t_begin, t_end = float(query["time"][0]), float(query["time"][-1])
    d_q = ctx.to_device(query)
    q_desc = R.Points(d_q.ptr, d_q.ptr + 24, 48, 48, len(query))
    d_xyz = ctx.alloc(12 * len(query))
    ident = (np.zeros(3), np.array([1.0, 0.0, 0.0, 0.0]))
    # the query sweep measured again from a moving sensor, as 48-byte records with its stamps
    pb = (np.array([0.02, -0.01, 0.005]), CT.quat_of_rotvec(np.deg2rad(0.5) * np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)))
    pe = CT.pose_update_ct(pb, np.array([0.004, -0.006, np.deg2rad(1.0), 0.04, 0.03, 0.0]))
    body, times = CT.simulate_sweep(xyz_of(query), pb, pe, t_begin, t_end)
    d_s = ctx.to_device(synth.make_points(body, times))
    s_desc = R.Points(d_s.ptr, d_s.ptr + 24, 48, 48, len(body))
    pb0 = CT.pose_update_ct(pb, np.array([0.002, -0.001, 0.002, 0.01, -0.015, 0.01]))
    pe0 = CT.pose_update_ct(pe, np.array([-0.002, 0.002, -0.001, -0.015, 0.01, -0.005]))
    out = dict(reps=reps, points_per_sweep=n_sweep, queries=len(query))
    for v in (0.05, 0.2):
        m = ctx.map_create(v, moments=True)
        for s in sweeps:
            m.insert(s)
        prm = lib.map_reg_params(v, 3, cauchy_a=0.4)

        def linearize(timer):
            if timer:
                ctx.timer_start()
            m.linearize_device(q_desc, np.eye(3, 4), prm)

        def linearize_ct(timer, xyz=None):
            if timer:
                ctx.timer_start()
            m.linearize_ct_device(q_desc, ident, ident, t_begin, t_end, prm, None, xyz)

        res = dict(voxels=m.size()[0])
        res["linearize_ms"] = timed(ctx, linearize, reps)
        res["linearize_ct_ms"] = timed(ctx, linearize_ct, reps)
        res["linearize_ct_xyz_ms"] = timed(ctx, lambda tm: linearize_ct(tm, d_xyz), reps)
        ne = m.linearize_ct_device(q_desc, ident, ident, t_begin, t_end, prm)
        res["used_rate"] = float(ne["n_used"]) / len(query)
        # both poses the identity: the moved point is the point itself, so the counts are the rigid call's (every workgroup here takes
        # several tiles: a count lost between two tiles of a workgroup shows up as a difference)
        ne_rigid = m.linearize_device(q_desc, np.eye(3, 4), prm)
        assert (int(ne["n_used"]), int(ne["n_found"]), int(ne["n_outside"])) == (int(ne_rigid["n_used"]), int(ne_rigid["n_found"]), 0)
        res["ct_over_rigid"] = res["linearize_ct_ms"]["median"] / res["linearize_ms"]["median"]
        res["ct_xyz_over_rigid"] = res["linearize_ct_xyz_ms"]["median"] / res["linearize_ms"]["median"]
        opts = lib.map_ct_align_opts(lib.map_reg_params(v, 3), max_iterations=30, tol_rot=1e-6, tol_trans=1e-5)
        m.align_ct_device(s_desc, pb0, pe0, t_begin, t_end, opts)  # (warm-up)
        ctx.sync()
        t0 = time.perf_counter()
        ctx.timer_start()
        b1, e1, summ = m.align_ct_device(s_desc, pb0, pe0, t_begin, t_end, opts)
        dev_ms = ctx.timer_stop_ms()
        wall_ms = 1e3 * (time.perf_counter() - t0)
        res["align_ct"] = dict(wall_ms=wall_ms, device_ms=dev_ms, iterations=summ["iterations"], termination=summ["termination"],
                               n_used=summ["n_used"], begin_error=CT.pose_error(b1, pb), end_error=CT.pose_error(e1, pe))
        out[f"v{v}"] = res
        print(v, json.dumps(res), file=sys.stderr, flush=True)
        m.close()
    for d in (d_q, d_xyz, d_s):
        d.free()
    ctx.close()
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
