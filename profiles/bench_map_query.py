"""Timings of the voxel map's query and crop (csrc/map.hip, include/wildcat_hip.h: wc_map_nearest, wc_map_crop).  Prints ONE JSON object:
  nearest     wc_map_nearest of 1 M queries (a fresh room sweep of 48-byte records, max_dist = v, count not requested) against the
              11-sweep map of bench_map.py at v = 0.05 and 0.2: the table as the inserts leave it ("as_inserted") and after an
              all-infinite crop ("compact"); device-timed (wc_timer_start / wc_timer_stop_ms) median and min of --reps calls after
              warm-up.  Per entry: table slots and bytes, hit rate, mean occupied neighbours per query
  bytes_per_query_from_shapes   27 key probes of 8 bytes + 32 bytes of payload per occupied neighbour + the 40-byte hit written + the
              48-byte query record; shape_GBps = that figure over the median time.  It counts the bytes the kernel asks for, not the
              sectors or lines the memory system moves for them
  crop_ms     wc_map_crop (host wall time: the call waits) of the as-inserted table for the all-infinite box and for a box that keeps
              about half of the voxels
  restatement_cpu_s   the numpy restatement (tests/map_query_ref.py) on the same queries and the exported map: the CPU baseline
  facade      LidarOdometry over the room stream of bench_map.py with the map on, and with map_keep_radius on top of it
python profiles/bench_map_query.py [--reps 20] [--quick]   (--quick: 3 repetitions, no facade and no CPU baseline)"""
import argparse
import ctypes as C
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "wildcat-slam_amd", "python"))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import numpy as np  # noqa: E402

import map_query_ref as Q  # noqa: E402
from map_bench_common import note, timed, xyz_of  # noqa: E402
from wildcat_slam_amd import lib, synth  # noqa: E402
from wildcat_slam_amd import records as R  # noqa: E402


def map_section(ctx, reps, baseline):
    n_sweep = 1_000_000
    sweeps = [synth.g1_room(n_sweep, seed=200 + i, t_start=1000.0 + 0.5 * i) for i in range(11)]
    query = synth.g1_room(n_sweep, seed=300, t_start=2000.0)
    dev = [ctx.to_device(s) for s in sweeps]
    desc = [R.Points(d.ptr, d.ptr + 24, 48, 48, len(s)) for d, s in zip(dev, sweeps)]
    d_q = ctx.to_device(query)
    q_desc = R.Points(d_q.ptr, d_q.ptr + 24, 48, 48, len(query))
    d_hits = ctx.alloc(R.MAP_HIT.itemsize * len(query))
    out = dict(queries=len(query))
    note("sweeps on the device")
    inf = float("inf")
    for v in (0.05, 0.2):
        m = ctx.map_create(v)

        def fill():
            m.clear()
            for k in range(11):
                ctx._ck(ctx.lib.wc_map_insert(ctx.h, m.h, C.byref(desc[k]), None))  # (back to back, as the facade inserts)

        def nearest(timer):
            if timer:
                ctx.timer_start()
            ctx._ck(ctx.lib.wc_map_nearest(ctx.h, m.h, C.byref(q_desc), C.c_double(v), C.c_void_p(d_hits.ptr), None))

        fill()
        cen, cnt, keys = m.export()
        note("v", v, "map filled and exported:", len(cnt), "voxels")
        # what a query meets: the occupied voxels among its 27 (on the host, from the exported keys)
        packed = Q.pack(keys)
        kq = Q.point_keys(xyz_of(query), v).astype(np.int64)
        occ = np.zeros(len(kq), np.int64)
        for off in np.ndindex(3, 3, 3):
            pk = Q.pack(kq + (np.array(off) - 1))
            pos = np.minimum(np.searchsorted(packed, pk), len(packed) - 1)
            occ += packed[pos] == pk
        entry = dict(voxels=len(cnt), mean_occupied_neighbours=float(occ.mean()))
        entry["bytes_per_query_from_shapes"] = round(27 * 8 + 32 * entry["mean_occupied_neighbours"] + 40 + 48, 1)
        for state in ("as_inserted", "compact"):
            if state == "compact":
                m.crop((-inf,) * 3, (inf,) * 3)
            info = m.info()
            t = timed(ctx, nearest, reps)
            med, mn = t["median"], t["min"]
            found = m.nearest_device(q_desc, v, d_hits)
            note("v", v, state, "nearest_ms", med, "slots", info["slots"])
            entry[state] = dict(table_slots=info["slots"], table_bytes=info["bytes"], nearest_ms=med, nearest_ms_min=mn,
                                hit_rate=found / len(query), shape_GBps=round(entry["bytes_per_query_from_shapes"] * len(query) / med / 1e6, 1))
        # crop: the as-inserted table, all-infinite box and a box that keeps about half (the voxels below the median x)
        half_x = float(np.median(cen[:, 0]))
        crops = {}
        for name, lo, hi in (("all_infinite", (-inf,) * 3, (inf,) * 3), ("keeps_half", (-inf,) * 3, (half_x, inf, inf))):
            ts, removed = [], 0
            for _ in range(max(3, reps // 4)):
                fill()
                ctx.sync()
                t0 = time.perf_counter()
                removed = m.crop(lo, hi)
                ts.append((time.perf_counter() - t0) * 1e3)
            note("v", v, "crop", name, ts)
            crops[name] = dict(ms_median=float(np.median(ts)), ms_min=float(np.min(ts)), removed_voxels=removed, slots_after=m.info()["slots"])
        entry["crop_ms"] = crops
        if baseline:
            t0 = time.perf_counter()
            Q.nearest_voxel(keys, cen, cnt, xyz_of(query), v, v)
            entry["restatement_cpu_s"] = time.perf_counter() - t0
        out[f"v{v}"] = entry
        m.close()
    for d in dev + [d_q, d_hits]:
        d.free()
    return out


def facade_section(duration, pps, voxel, radius):
    msgs, imu, _ = synth.raw_stream(duration, pts_per_s=pps, gyro_bias=(0.0, 0.0, 0.02), t_start=1000.0)
    note("facade stream ready")
    res = {}
    for name, r in (("map_on", 0.0), ("map_keep_radius", radius)):
        odo = lib.Odometry(0)
        odo.set_map_voxel(voxel)
        odo.set_map_keep_radius(r)
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
        res[name] = dict(sweeps=len(times), median_ms=float(np.median(times[2:])), map_step_median_ms=float(np.median(map_ms[2:])))
        res[name]["map_voxels"], res[name]["map_points"], _ = odo.map_size()
        note("facade", name, res[name])
        odo.close()
    res["radius"], res["voxel"], res["points_per_sweep"] = radius, voxel, int(pps * 0.5)
    res["parent_map_step_median_ms"] = 0.052  # profiles/map_bench.json, before map_keep_radius existed
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    reps = 3 if a.quick else max(20, a.reps)
    ctx = lib.Context(0)
    out = dict(reps=reps, map=map_section(ctx, reps, not a.quick))
    ctx.close()
    if not a.quick:
        out["facade"] = facade_section(8.9, 600_000, 0.1, 10.0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
