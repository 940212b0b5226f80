"""Timings of the voxel map's k-nearest query (csrc/map.hip, include/wildcat_hip.h: wc_map_knn).  Prints ONE JSON object:
  per voxel size (0.05 and 0.2): the 11-sweep room map of bench_map.py after an all-infinite crop (the compact table), queried with
  1 M points of a fresh room sweep (48-byte records), counts not requested:
    nearest     wc_map_nearest at max_dist = v: the yardstick, with its own run-to-run spread ((max - min) / median of the timed calls)
    knn         wc_map_knn for k in {1, 4, 8, 16} x reach in {1, 2} at max_dist = reach * v, min_points = 1, with d_within: median, min
                and max, the mean of within and of the records written per query
    k1_reach1_over_nearest   the ratio of the medians of the k = 1 / reach = 1 call and of wc_map_nearest
    ms_per_extra_k           per reach: (median at k = 16 - median at k = 1) / 15
    reach_step_ratio         per k: median at reach 2 over median at reach 1
  device-timed (wc_timer_start / wc_timer_stop_ms) after warm-up.
python profiles/bench_map_knn.py [--reps 20] [--quick]   (--quick: 3 repetitions, 3 sweeps of 200 k points)"""
import argparse
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "wildcat-slam_amd", "python"))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import numpy as np  # noqa: E402

from map_bench_common import note  # noqa: E402
from wildcat_slam_amd import lib, synth  # noqa: E402
from wildcat_slam_amd import records as R  # noqa: E402

KS, REACHES = (1, 4, 8, 16), (1, 2)


def spread(ctx, fn, reps, warmup=3):
    """median, min and max [ms] of `reps` device-timed calls of fn() after `warmup` untimed ones"""
    for _ in range(warmup):
        fn()
        ctx.sync()
    ts = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        ts.append(ctx.timer_stop_ms())
    return dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), max_ms=float(np.max(ts)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    reps = 3 if a.quick else max(20, a.reps)
    n_sweep, n_sweeps = (200_000, 3) if a.quick else (1_000_000, 11)
    ctx = lib.Context(0)
    sweeps = [synth.g1_room(n_sweep, seed=200 + i, t_start=1000.0 + 0.5 * i) for i in range(n_sweeps)]
    query = synth.g1_room(n_sweep, seed=300, t_start=2000.0)
    n = len(query)
    d_q = ctx.to_device(query)
    q_desc = R.Points(d_q.ptr, d_q.ptr + 24, 48, 48, n)
    d_hits, d_within = ctx.alloc(R.MAP_HIT.itemsize * n * max(KS)), ctx.alloc(4 * n)
    note("sweeps and queries ready")
    inf = float("inf")
    out = dict(reps=reps, queries=n, sweeps=n_sweeps)
    for v in (0.05, 0.2):
        m = ctx.map_create(v)
        for s in sweeps:
            m.insert(s)
        m.crop((-inf,) * 3, (inf,) * 3)
        info = m.info()
        entry = dict(voxels=m.size()[0], table_slots=info["slots"], table_bytes=info["bytes"])
        note("v", v, entry)

        def nearest():
            ctx._ck(ctx.lib.wc_map_nearest(ctx.h, m.h, C.byref(q_desc), C.c_double(v), C.c_void_p(d_hits.ptr), None))

        near = spread(ctx, nearest, reps)
        near["spread"] = (near["max_ms"] - near["min_ms"]) / near["median_ms"]
        near["hit_rate"] = m.nearest_device(q_desc, v, d_hits) / n
        entry["nearest"] = near
        note("v", v, "nearest", near)
        knn = {}
        for reach in REACHES:
            for k in KS:
                params = R.MapKnnParams(reach * v, k, reach, 1, 0)

                def call():
                    m.knn_device(q_desc, params, d_hits, d_within, want_counts=False)

                t = spread(ctx, call, reps)
                some, rec, total = m.knn_device(q_desc, params, d_hits, d_within)
                t.update(mean_within=total / n, mean_records=rec / n, queries_with_a_neighbour=some / n)
                knn[f"k{k}_reach{reach}"] = t
                note("v", v, "k", k, "reach", reach, t)
        entry["knn"] = knn
        entry["k1_reach1_over_nearest"] = knn["k1_reach1"]["median_ms"] / near["median_ms"]
        entry["ms_per_extra_k"] = {f"reach{r}": (knn[f"k16_reach{r}"]["median_ms"] - knn[f"k1_reach{r}"]["median_ms"]) / 15 for r in REACHES}
        entry["reach_step_ratio"] = {f"k{k}": knn[f"k{k}_reach2"]["median_ms"] / knn[f"k{k}_reach1"]["median_ms"] for k in KS}
        out[f"v{v}"] = entry
        m.close()
    for d in (d_q, d_hits, d_within):
        d.free()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
