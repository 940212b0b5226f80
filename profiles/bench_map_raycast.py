"""Timings of wc_map_raycast (csrc/map.hip: k_map_raycast) beside wc_map_carve of the same rays.  Writes profiles/map_raycast_bench.json
(--out) after every step, so that a run that does not complete leaves what it measured:
  the map      ONE one-million-point room sweep (synth.g1_room) inserted once into a map created with reserve_voxels = 2^20, at v = 0.2
               and 0.05: no growth, no clear, no crop, no second insert
  cast_ms      a second sweep of that room as rays from the sensor's position in the middle of it, max_range 30 m: first every tenth
               point (100 k rays, a strided call), then all of them (1 M), at end_shell 0 and 2; median and minimum of --reps
               device-timed calls (wc_timer_start / wc_timer_stop_ms around the whole call: the counters' memset, the kernel and the
               read-back); tested_per_s = the call's `tested` counter over the median
  carve_ms     wc_map_carve of the same rays (shell 1, min_rays 2), the same way; steps_per_s = its `steps` counter over the median
  cpu          the numpy restatement (tests/map_raycast_ref.py) on 10 k rays against the map's export, wall time
One process; every step runs under its own alarm (--step-limit seconds, default action: the process ends there).
python profiles/bench_map_raycast.py [--reps 5] [--step-limit 60] [--out profiles/map_raycast_bench.json]"""
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

import map_raycast_ref as RR  # noqa: E402
from map_bench_common import xyz_of  # noqa: E402
from wildcat_slam_amd import lib, synth  # noqa: E402
from wildcat_slam_amd import records as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-limit", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(HERE, "map_raycast_bench.json"))
    a = ap.parse_args()
    out = dict(reps=a.reps, max_range=30.0, complete=False, steps_done=[])
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
    sweep, rays = step("sweeps", lambda: (synth.g1_room(n_sweep, seed=200, t_start=1000.0), synth.g1_room(n_sweep, seed=300, t_start=1005.5)))
    origin = synth.traj_pos(0.25) + np.array([0.0, 0.0, 1.5])
    d_sweep, d_rays = ctx.to_device(sweep), ctx.to_device(rays)
    sweep_desc = R.Points(d_sweep.ptr, d_sweep.ptr + 24, 48, 48, len(sweep))
    n_of = {"100k": (len(rays) + 9) // 10, "1M": len(rays)}
    ray_desc = {"100k": R.Points(d_rays.ptr, 0, 480, 0, n_of["100k"]), "1M": R.Points(d_rays.ptr, 0, 48, 0, n_of["1M"])}
    d_hits = ctx.alloc(48 * len(rays))
    xyz = xyz_of(rays)
    out["points_per_sweep"] = len(rays)
    for v in (0.2, 0.05):
        m = ctx.map_create(v, reserve_voxels=1 << 20)
        sec = out.setdefault(f"v{v}", {"100k": {}, "1M": {}})

        def build():
            ctx._ck(ctx.lib.wc_map_insert(ctx.h, m.h, C.byref(sweep_desc), None))
            voxels, info = m.size()[0], m.info()
            say("map built:", voxels, "voxels,", info["slots"], "slots,", info["growths"], "growths")
            return dict(voxels=voxels, slots=info["slots"], growths=info["growths"])

        def cast(which, end_shell):
            params = lib.map_raycast_params(30.0, 0.0, 0, end_shell, 1, 4096)
            ms, res = [], None
            for rep in range(a.reps + 1):  # (the first call takes the counters' scratch: not timed)
                ctx.timer_start()
                res = m.raycast_device(ray_desc[which], origin, params, d_hits)
                ms.append(ctx.timer_stop_ms())
                say("cast", which, "end_shell", end_shell, "rep", rep, "%.3f ms" % ms[-1])
            med = float(np.median(ms[1:]))
            return {f"end_shell_{end_shell}": dict(cast_ms=med, cast_ms_min=float(np.min(ms[1:])), tested_per_s=res["tested"] / (med * 1e-3),
                                                   rays_per_s=n_of[which] / (med * 1e-3), **res)}

        def carve(which):
            params = lib.map_carve_params(30.0, 0.0, 1, 2, 4096)
            ms, res = [], None
            for rep in range(a.reps + 1):  # (the first call takes the scratch: not timed)
                ctx.timer_start()
                res = m.carve_device(ray_desc[which], origin, params)
                ms.append(ctx.timer_stop_ms())
                say("carve", which, "rep", rep, "%.3f ms" % ms[-1])
            med = float(np.median(ms[1:]))
            return dict(carve_ms=med, carve_ms_min=float(np.min(ms[1:])), steps_per_s=res["steps"] / (med * 1e-3), rays_used=res["rays_used"],
                        steps=res["steps"], voxels_selected=res["voxels_removed"])

        sec["map"] = step(f"v{v} build", build)
        for which in ("100k", "1M"):
            for end_shell in (0, 2):
                step(f"v{v} cast {which} end_shell {end_shell}", lambda: cast(which, end_shell), sec[which])
        for which in ("100k", "1M"):
            step(f"v{v} carve {which}", lambda: carve(which), sec[which])

        def cpu():
            cen, cnt, keys = m.export()
            sub = xyz[:: len(xyz) // 10_000][:10_000]
            t0 = time.perf_counter()
            _, res = RR.raycast(keys, cnt, cen, sub, origin, v, 30.0, end_shell=2)
            dt = time.perf_counter() - t0
            return dict(rays=len(sub), end_shell=2, seconds=dt, tested_per_s=res["tested"] / dt, **res)

        sec["cpu_numpy_10k"] = step(f"v{v} cpu", cpu)
        m.close()
    out["complete"] = True
    step("done", dict)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
