"""Timings of the device-resident voxel map (csrc/map.hip, include/wildcat_hip.h: wc_map_*).  Prints ONE JSON object:
  insert_ms   one 1 M-point sweep of 48-byte records (the room of synth.g1_room) into an empty map, and into a map that already holds
              10 such sweeps, at v = 0.05 and 0.2 (median of --reps device-timed calls, wc_timer_start / wc_timer_stop_ms, after warm-up)
  export_ms   wc_map_export of the 11-sweep map (the size read-back included)
  voxels, bytes per point from the shapes (the 48-byte record read once, 40 bytes of table per distinct voxel of the call: 8 of key
              probe + 32 of integer atomics - a lower bound, a voxel met by several tiles is probed once per tile)
  facade      per-sweep wall time of LidarOdometry::AddLidarScan (median) over the room stream of synth.raw_stream with the map off and on
python profiles/bench_map.py [--reps 20] [--quick]   (--quick: 3 repetitions and no facade section, for a kernel trace)"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "wildcat-slam_amd", "python"))
import numpy as np  # noqa: E402

from map_bench_common import timed  # noqa: E402
from wildcat_slam_amd import lib, synth  # noqa: E402
from wildcat_slam_amd import records as R  # noqa: E402


def map_section(ctx, reps):
    n_sweep = 1_000_000
    sweeps = [synth.g1_room(n_sweep, seed=200 + i, t_start=1000.0 + 0.5 * i) for i in range(11)]
    dev = [ctx.to_device(s) for s in sweeps]
    desc = [R.Points(d.ptr, d.ptr + 24, 48, 48, len(s)) for d, s in zip(dev, sweeps)]
    out = dict(points_per_sweep=[len(s) for s in sweeps[:1]][0])
    for v in (0.05, 0.2):
        m = ctx.map_create(v)
        insert = ctx.lib.wc_map_insert

        def one(timer, prefill):
            ctx._ck(ctx.lib.wc_map_clear(ctx.h, m.h))
            for k in range(prefill):
                ctx._ck(insert(ctx.h, m.h, C.byref(desc[k]), None))
            m.size()  # (the occupied count exact: the timed call never grows the table after the warm-up)
            if timer:
                ctx.timer_start()
            ctx._ck(insert(ctx.h, m.h, C.byref(desc[10]), None))

        empty = timed(ctx, lambda c: one(c, 0), reps)
        voxels_1 = m.size()[0]
        full = timed(ctx, lambda c: one(c, 10), reps)
        voxels_11 = m.size()[0]
        ctx._ck(ctx.lib.wc_map_clear(ctx.h, m.h))
        for k in range(10):
            ctx._ck(insert(ctx.h, m.h, C.byref(desc[k]), None))
        voxels_10 = m.size()[0]
        ctx._ck(insert(ctx.h, m.h, C.byref(desc[10]), None))
        n = m.size()[0]
        bx, bc, bk = ctx.alloc(12 * n), ctx.alloc(4 * n), ctx.alloc(12 * n)

        def exp(timer):
            if timer:
                ctx.timer_start()
            rc, _ = m.export_device(bx, bc, bk, n)
            ctx._ck(rc)

        ex = timed(ctx, exp, reps)
        info = m.info()
        out[f"v{v}"] = dict(
            insert_ms_empty=empty["median"], insert_ms_empty_min=empty["min"], insert_ms_10_sweeps=full["median"], insert_ms_10_sweeps_min=full["min"],
            export_ms=ex["median"], voxels_one_sweep=voxels_1, voxels_10_sweeps=voxels_10, voxels_11_sweeps=voxels_11,
            new_voxels_in_timed_insert=voxels_11 - voxels_10, table_slots=info["slots"], table_growths=info["growths"],
            bytes_per_point_input=48, bytes_per_point_table_lower_bound=round(40.0 * voxels_1 / len(sweeps[10]), 2))
        for b in (bx, bc, bk):
            b.free()
        m.close()
    for d in dev:
        d.free()
    return out


def facade_section(duration, pps, voxel):
    msgs, imu, _ = synth.raw_stream(duration, pts_per_s=pps, gyro_bias=(0.0, 0.0, 0.02), t_start=1000.0)
    res = {}
    for name, v in (("map_off", 0.0), ("map_on", voxel)):
        odo = lib.Odometry(0)
        if v:
            odo.set_map_voxel(v)
        k, times, map_ms, before = 0, [], [], 0
        for msg in msgs:
            if len(msg) == 0:
                continue
            while k < len(imu["t"]) and imu["t"][k] <= msg["time"][-1] + 0.02:
                odo.add_imu(imu["t"][k], imu["acc"][k], imu["gyr"][k])
                k += 1
            t0 = time.perf_counter()
            odo.add_scan(msg)
            dt = time.perf_counter() - t0
            if odo.sweeps() > before:
                before = odo.sweeps()
                times.append(dt * 1e3)
                map_ms.append(odo.map_ms())
        res[name] = dict(sweeps=len(times), median_ms=float(np.median(times[2:])), max_ms=float(np.max(times[2:])),
                         map_step_median_ms=float(np.median(map_ms[2:])))
        if v:
            res[name]["map_voxels"], res[name]["map_points"], res[name]["map_rejected"] = odo.map_size()
        odo.close()
    res["delta_median_ms"] = res["map_on"]["median_ms"] - res["map_off"]["median_ms"]
    res["points_per_sweep"] = int(pps * 0.5)
    res["voxel"] = voxel
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    reps = 3 if a.quick else max(20, a.reps)
    ctx = lib.Context(0)
    out = dict(reps=reps, map=map_section(ctx, reps))
    ctx.close()
    if not a.quick:
        out["facade"] = facade_section(8.9, 600_000, 0.1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
