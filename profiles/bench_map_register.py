"""Timings of the registration against the voxel map (csrc/map.hip: k_map_linearize<true>, k_map_lin_reduce; include/wildcat_hip.h
"registration against the map") beside the plane query it grew out of, in one process, on the 11-sweep map of bench_map_surfels.py
(1 M-point sweeps of the room of synth.g1_room, v = 0.05 and 0.2).  Prints ONE JSON object and writes it to
profiles/map_register_bench.json:
  nearest_plane_ms   wc_map_nearest_plane (min_points 3, max_dist v, no count read-back) of 1 M queries: 80 bytes written per query
  linearize_ms       wc_map_linearize of the same 1 M points at the identity pose, the Cauchy loss on (a = 0.4), without and with d_rows:
                     the same search, 0 (64) bytes written per point, the reduction launches and the 240-byte read-back inside the timed span
  align              one wc_map_align of the query sweep moved by the inverse of a pose 0.5 degrees and 2 cm off: wall and device time of
                     the whole loop, iterations, termination and the pose error left
Every device figure: median and minimum of --reps device-timed calls (wc_timer_start / wc_timer_stop_ms) after 3 warm-up calls.
python profiles/bench_map_register.py [--reps 20] [--out profiles/map_register_bench.json]"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "wildcat-slam_amd", "python"))
import numpy as np  # noqa: E402

from map_bench_common import timed, xyz_of  # noqa: E402
from wildcat_slam_amd import lib, synth  # noqa: E402
from wildcat_slam_amd import records as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(HERE, "map_register_bench.json"))
    a = ap.parse_args()
    reps = max(3, a.reps)
    ctx = lib.Context(0)
    n_sweep = 1_000_000
    sweeps = [synth.g1_room(n_sweep, seed=200 + i, t_start=1000.0 + 0.5 * i) for i in range(11)]
    query = synth.g1_room(n_sweep, seed=300, t_start=2000.0)
    d_q = ctx.to_device(query)
    q_desc = R.Points(d_q.ptr, d_q.ptr + 24, 48, 48, len(query))
    d_hits = ctx.alloc(R.MAP_PLANE_HIT.itemsize * len(query))
    d_rows = ctx.alloc(R.MAP_REG_ROW.itemsize * len(query))
    # the query sweep as a scan: moved by the inverse of a small pose, packed xyz
    w = np.deg2rad(0.5) * np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    th = np.linalg.norm(w)
    Rm = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th**2 * (K @ K)
    t = np.array([0.02, -0.01, 0.005])
    xyz = xyz_of(query).astype(np.float64)
    scan = ((xyz - t) @ Rm).astype(np.float32)
    d_s = ctx.to_device(scan)
    s_desc = R.Points(d_s.ptr, 0, 12, 0, len(scan))
    identity = np.eye(3, 4)
    out = dict(reps=reps, points_per_sweep=n_sweep, queries=len(query))
    for v in (0.05, 0.2):
        m = ctx.map_create(v, moments=True)
        for s in sweeps:
            m.insert(s)
        prm = lib.map_reg_params(v, 3, cauchy_a=0.4)

        def nearest_plane(timer):
            if timer:
                ctx.timer_start()
            m.nearest_plane_device(q_desc, v, 3, d_hits, want_count=False)

        def linearize(timer, rows=None):
            if timer:
                ctx.timer_start()
            m.linearize_device(q_desc, identity, prm, rows)

        res = dict(voxels=m.size()[0])
        res["nearest_plane_ms"] = timed(ctx, nearest_plane, reps)
        res["linearize_ms"] = timed(ctx, linearize, reps)
        res["linearize_rows_ms"] = timed(ctx, lambda tm: linearize(tm, d_rows), reps)
        ne = m.linearize_device(q_desc, identity, prm)
        res["used_rate"] = float(ne["n_used"]) / len(query)
        res["linearize_over_nearest_plane"] = res["linearize_ms"]["median"] / res["nearest_plane_ms"]["median"]
        opts = lib.map_align_opts(lib.map_reg_params(v, 3), max_iterations=30, tol_rot=1e-7, tol_trans=1e-6)
        m.align_device(s_desc, identity, opts)  # (warm-up)
        ctx.sync()
        t0 = time.perf_counter()
        ctx.timer_start()
        T, summ = m.align_device(s_desc, identity, opts)
        dev_ms = ctx.timer_stop_ms()
        wall_ms = 1e3 * (time.perf_counter() - t0)
        dR = T[:, :3] @ Rm.T
        ang = float(np.arccos(np.clip(0.5 * (np.trace(dR) - 1), -1, 1)))
        res["align"] = dict(wall_ms=wall_ms, device_ms=dev_ms, iterations=summ["iterations"], termination=summ["termination"],
                            n_used=summ["n_used"], rot_error_rad=ang, trans_error_m=float(np.linalg.norm(T[:, 3] - t)))
        out[f"v{v}"] = res
        print(v, json.dumps(res), file=sys.stderr, flush=True)
        m.close()
    for d in (d_q, d_hits, d_rows, d_s):
        d.free()
    ctx.close()
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
