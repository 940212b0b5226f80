"""Timings of the voxel map's surfels (WC_MAP_MOMENTS: csrc/map.hip, include/wildcat_hip.h "map surfels") beside the plain map, in one
process, on the clouds and voxel sizes of bench_map.py (1 M-point sweeps of the room of synth.g1_room, v = 0.05 and 0.2).  Prints ONE
JSON object and writes it to profiles/map_surfel_bench.json:
  insert_ms      one sweep into an empty map and into a map that holds 10 sweeps: plain, moments with the insert's two forms (the
                 development option map_mom_pts: 1 = 256-point tiles and 54 KB of LDS, 2 = the plain insert's 512-point tiles and 108 KB)
  export_ms      wc_map_export and wc_map_export_surfels of the 11-sweep map (the size read-back included)
  nearest_ms     wc_map_nearest and wc_map_nearest_plane (min_points 3) for 1 M queries within v of the 11-sweep map
Every figure: median and minimum of --reps device-timed calls (wc_timer_start / wc_timer_stop_ms) after 3 warm-up calls.
python profiles/bench_map_surfels.py [--reps 20] [--out profiles/map_surfel_bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "wildcat-slam_amd", "python"))
import numpy as np  # noqa: E402

from map_bench_common import timed  # noqa: E402
from wildcat_slam_amd import lib, synth  # noqa: E402
from wildcat_slam_amd import records as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(HERE, "map_surfel_bench.json"))
    a = ap.parse_args()
    reps = max(3, a.reps)
    ctx = lib.Context(0)
    n_sweep = 1_000_000
    sweeps = [synth.g1_room(n_sweep, seed=200 + i, t_start=1000.0 + 0.5 * i) for i in range(11)]
    query = synth.g1_room(n_sweep, seed=300, t_start=2000.0)
    dev = [ctx.to_device(s) for s in sweeps]
    desc = [R.Points(d.ptr, d.ptr + 24, 48, 48, len(s)) for d, s in zip(dev, sweeps)]
    d_q = ctx.to_device(query)
    q_desc = R.Points(d_q.ptr, d_q.ptr + 24, 48, 48, len(query))
    d_hits = ctx.alloc(R.MAP_PLANE_HIT.itemsize * len(query))
    insert = ctx.lib.wc_map_insert
    out = dict(reps=reps, points_per_sweep=n_sweep, queries=len(query))
    for v in (0.05, 0.2):
        entry = {}
        forms = (("plain", False, 1), ("moments_tile256", True, 1), ("moments_tile512", True, 2))
        for name, moments, pts in forms:
            ctx.set_dev_option("map_mom_pts", pts)
            m = ctx.map_create(v, moments=moments)

            def one(timer, prefill):
                m.clear()
                for k in range(prefill):
                    ctx._ck(insert(ctx.h, m.h, C.byref(desc[k]), None))
                m.size()  # (the occupied count exact: the timed call never grows the table after the warm-up)
                if timer:
                    ctx.timer_start()
                ctx._ck(insert(ctx.h, m.h, C.byref(desc[10]), None))

            res = dict(insert_ms_empty=timed(ctx, lambda t: one(t, 0), reps), insert_ms_10_sweeps=timed(ctx, lambda t: one(t, 10), reps))
            n = m.size()[0]
            info = m.info()
            res.update(voxels=n, table_slots=info["slots"], table_bytes=info["bytes"])
            if name != "moments_tile512":  # (export and query do not depend on the insert's form)
                bx, bc, bk, bs = ctx.alloc(12 * n), ctx.alloc(4 * n), ctx.alloc(12 * n), ctx.alloc(128 * n)

                def export(timer):
                    if timer:
                        ctx.timer_start()
                    ctx._ck(m.export_device(bx, bc, bk, n)[0])

                def export_surfels(timer):
                    if timer:
                        ctx.timer_start()
                    ctx._ck(m.surfels_device(bs, n)[0])

                def nearest(timer):
                    if timer:
                        ctx.timer_start()
                    m.nearest_device(q_desc, v, d_hits, want_count=False)

                def nearest_plane(timer):
                    if timer:
                        ctx.timer_start()
                    m.nearest_plane_device(q_desc, v, 3, d_hits, want_count=False)

                res["export_ms"] = timed(ctx, export, reps)
                res["nearest_ms"] = timed(ctx, nearest, reps)
                if moments:
                    res["export_surfels_ms"] = timed(ctx, export_surfels, reps)
                    res["nearest_plane_ms"] = timed(ctx, nearest_plane, reps)
                    hits = d_hits.download(R.MAP_PLANE_HIT, len(query))
                    res["hit_rate"] = float((hits["count"] > 0).mean())
                    res["plane_rate"] = float(((hits["flags"] & 2) != 0).mean())
                for b in (bx, bc, bk, bs):
                    b.free()
            entry[name] = res
            print(v, name, json.dumps(res), file=sys.stderr, flush=True)
            m.close()
        ctx.set_dev_option("map_mom_pts", 1)
        p, a256, a512 = (entry[k]["insert_ms_10_sweeps"]["median"] for k in ("plain", "moments_tile256", "moments_tile512"))
        entry["insert_ratio_tile256_over_plain"] = a256 / p
        entry["insert_ratio_tile512_over_plain"] = a512 / p
        out[f"v{v}"] = entry
    for d in dev + [d_q, d_hits]:
        d.free()
    ctx.close()
    text = json.dumps(out, indent=1)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
