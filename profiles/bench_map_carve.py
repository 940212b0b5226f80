"""Timings of wc_map_carve (csrc/map.hip: k_map_carve, then the count of what it selects).  Writes profiles/map_carve_bench.json
(--out) after every step, so that a run that does not complete leaves what it measured:
  the map      the 11 one-million-point room sweeps of profiles/bench_map.py at v = 0.2 and 0.05
  walk_ms      one more sweep of that room as rays from the sensor's position in the middle of it, max_range 30 m, shell 1: first every
               tenth point (100 k rays, a strided call), then all of them (1 M); median and minimum of --reps device-timed calls
               (wc_timer_start / wc_timer_stop_ms around the whole call: the scratch's memset, the ray kernel, the count and the
               read-back) with min_rays 2; steps_per_s = the call's `steps` counter over the median
  insert_ms    wc_map_insert of the same sweep into the same map, beside it (after the first call the voxel set no longer changes)
  cpu          the numpy restatement (tests/map_carve_ref.py: through_counts) on 10 k rays at the same voxel size and range, wall time
One process; every step runs under its own alarm (--step-limit seconds, default action: the process ends there).
python profiles/bench_map_carve.py [--reps 5] [--step-limit 60] [--out profiles/map_carve_bench.json]"""
import argparse
import ctypes as C
import json
import os
import signal
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "wildcat-slam_amd", "python"))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import numpy as np  # noqa: E402

import map_carve_ref as CR  # noqa: E402
from map_bench_common import xyz_of  # noqa: E402
from wildcat_slam_amd import lib, synth  # noqa: E402
from wildcat_slam_amd import records as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-limit", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(HERE, "map_carve_bench.json"))
    a = ap.parse_args()
    out = dict(reps=a.reps, max_range=30.0, shell=1, complete=False, steps_done=[])
    t_start = time.perf_counter()

    def say(*what):
        print("[%7.2f s]" % (time.perf_counter() - t_start), *what, flush=True)

    def step(name, fn, into=None):
        say("step", name)
        signal.alarm(a.step_limit)  # (default action: a step that hangs ends the process; the file holds what was measured)
        res = fn()
        signal.alarm(0)
        if into is not None:
            into.update(res)
        out["steps_done"].append(name)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
        return res

    ctx = lib.Context(0)
    n_sweep = 1_000_000
    sweeps = step("sweeps", lambda: [synth.g1_room(n_sweep, seed=200 + i, t_start=1000.0 + 0.5 * i) for i in range(11)])
    rays = synth.g1_room(n_sweep, seed=300, t_start=1005.5)
    origin = synth.traj_pos(0.25) + np.array([0.0, 0.0, 1.5])
    dev = [ctx.to_device(s) for s in sweeps]
    desc = [R.Points(d.ptr, d.ptr + 24, 48, 48, len(s)) for d, s in zip(dev, sweeps)]
    d_rays = ctx.to_device(rays)
    ray_desc = {"100k": R.Points(d_rays.ptr, 0, 480, 0, (len(rays) + 9) // 10), "1M": R.Points(d_rays.ptr, 0, 48, 0, len(rays))}
    xyz = xyz_of(rays)
    out["points_per_sweep"] = len(rays)
    for v in (0.2, 0.05):
        m = ctx.map_create(v)
        sec = out.setdefault(f"v{v}", {"100k": {}, "1M": {}})

        def rebuild():
            ctx._ck(ctx.lib.wc_map_clear(ctx.h, m.h))
            for k in range(11):
                ctx._ck(ctx.lib.wc_map_insert(ctx.h, m.h, C.byref(desc[k]), None))
            voxels = m.size()[0]
            say("map rebuilt:", voxels, "voxels,", m.info()["slots"], "slots")
            return voxels

        def walk(which):
            params = lib.map_carve_params(30.0, 0.0, 1, 2, 4096)
            ms, res = [], None
            for rep in range(a.reps + 1):  # (the first call takes the scratch: not timed)
                ctx.timer_start()
                res = m.carve_device(ray_desc[which], origin, params)
                ms.append(ctx.timer_stop_ms())
                say("walk", which, "rep", rep, "%.3f ms" % ms[-1])
            med = float(np.median(ms[1:]))
            return dict(walk_ms=med, walk_ms_min=float(np.min(ms[1:])), steps_per_s=res["steps"] / (med * 1e-3), rays_used=res["rays_used"],
                        rays_skipped=res["rays_skipped"], steps=res["steps"], voxels_selected=res["voxels_removed"])

        def insert(which):
            ms = []
            for rep in range(a.reps + 1):
                ctx.timer_start()
                ctx._ck(ctx.lib.wc_map_insert(ctx.h, m.h, C.byref(ray_desc[which]), None))
                ms.append(ctx.timer_stop_ms())
            say("insert", which, ["%.3f" % t for t in ms])
            return dict(insert_ms=float(np.median(ms[1:])), insert_ms_min=float(np.min(ms[1:])))

        sec["voxels_11_sweeps"] = step(f"v{v} build", rebuild)
        for which in ("100k", "1M"):
            step(f"v{v} walk {which}", lambda: walk(which), sec[which])
        for which in ("100k", "1M"):
            step(f"v{v} insert {which}", lambda: insert(which), sec[which])

        def cpu():
            sub = xyz[:: len(xyz) // 10_000][:10_000]
            t0 = time.perf_counter()
            _, _, _, r = CR.through_counts(sub, origin, v, 30.0, 0.0, 1, 4096)
            dt = time.perf_counter() - t0
            return dict(rays=len(sub), steps=int(r["M"].sum()), seconds=dt, steps_per_s=float(r["M"].sum()) / dt)

        sec["cpu_numpy_10k"] = step(f"v{v} cpu", cpu)
        m.close()
    out["complete"] = True
    step("done", dict)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
