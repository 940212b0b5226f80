"""Timings of the batched registration (csrc/map.hip: k_map_linearize<false>, k_map_lin_reduce) beside the single calls
it replaces.  Writes profiles/map_align_batch_bench.json (--out) after every step, so that a run that does not complete leaves what it
measured:
  the map      DESIGN 8.9's room (60 000 points, v = 0.2) and its three coarser levels
  the scans    g1_room(n, seed + 7), n = 4000 and 48 000, in the sensor frame of tests/map_search_ref.py's true pose; the starts are
               the K yaw hypotheses of (I | c), K = 1, 8 and 64
  align        PointMap.align_batch_device of the K starts against the v = 0.8 level beside K single align_device calls of the same
               starts (10 iterations at most, the tolerances of the tests)
  pyramid      map_align_pyramid_batch_device through the four levels beside K single map_align_pyramid_device calls
               each the median and minimum of --reps device-timed runs (wc_timer_start / wc_timer_stop_ms around the whole call, or
               around the K single calls) after one untimed run; rounds = the largest iteration count of a hypothesis + 1
  check        what was timed is what the tests check: the batched poses equal the single calls' byte for byte
One process; every step runs under its own alarm (--step-limit seconds, default action: the process ends there), and the first step
that fails ends the run.  No figure is a pass condition.
python profiles/bench_map_align_batch.py [--reps 20] [--step-limit 120] [--out profiles/map_align_batch_bench.json]"""
import argparse
import json
import os
import signal
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "wildcat-slam_amd", "python"))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import numpy as np  # noqa: E402

import map_coarsen_ref as MC  # noqa: E402
import map_register_ref as G  # noqa: E402
import map_search_ref as MS  # noqa: E402
from map_bench_common import xyz_of  # noqa: E402
from wildcat_slam_amd import lib, synth  # noqa: E402
from wildcat_slam_amd import records as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-limit", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(HERE, "map_align_batch_bench.json"))
    a = ap.parse_args()
    out = dict(reps=a.reps, complete=False, steps_done=[])
    t_start = time.perf_counter()

    def say(*what):
        print("[%7.2f s]" % (time.perf_counter() - t_start), *what, flush=True)

    def step(name, fn):
        say("step", name)
        signal.alarm(a.step_limit)  # (default action: a step that hangs ends the process; the file holds what was measured)
        res = fn()
        signal.alarm(0)
        out["steps_done"].append(name)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
        return res

    ctx = lib.Context(0)
    world = {}

    def build():
        fine = ctx.map_create(MC.BASIN_V, moments=True)
        fine.insert(xyz_of(synth.g1_room(MC.BASIN_ROOM)))
        world["levels"] = fine.pyramid(MC.BASIN_FACTOR, MC.BASIN_LEVELS)[::-1]  # coarsest first
        return {f"v{m.voxel}": dict(voxels=m.size()[0]) for m in world["levels"]}

    out["maps"] = step("build", build)
    levels = world["levels"]
    kw = dict(max_iterations=MS.SEARCH_ITERS, tol_rot=G.TOL_ROT, tol_trans=G.TOL_TRANS)
    pyr_opts = lib.map_pyramid_opts(levels, **kw)
    m08 = levels[1]
    opts08 = pyr_opts[1]
    T_true = MS.search_pose()

    def timed(call):
        ms, res = [], None
        for _ in range(a.reps + 1):
            ctx.sync()
            ctx.timer_start()
            res = call()
            ms.append(ctx.timer_stop_ms())
        return dict(ms=float(np.median(ms[1:])), ms_min=float(np.min(ms[1:]))), res

    for n in (4000, 48_000):
        p = xyz_of(synth.g1_room(n, seed=synth.SEED + 7)).astype(np.float64)
        scan = ((p - T_true[:, 3]) @ T_true[:, :3]).astype(np.float32)
        d = ctx.to_device(scan)
        desc = R.Points(d.ptr, 0, 12, 0, n)
        for K in (1, 8, 64):
            starts = lib.pose_yaw_grid(MS.search_start(), K)
            sec = out.setdefault(f"n{n}_K{K}", {})

            def align():
                batch, (Tb, sb, stb) = timed(lambda: m08.align_batch_device(desc, starts, opts08))
                single, Ts = timed(lambda: [m08.align_device(desc, T, opts08)[0] for T in starts])
                assert not stb.any() and Tb.tobytes() == np.stack(Ts).tobytes()
                return dict(batch=batch, singles=single, speedup=single["ms"] / batch["ms"], rounds=max(s["iterations"] for s in sb) + 1,
                            linearisations=sum(s["iterations"] + (s["termination"] != 2) for s in sb), poses_equal=True)

            sec["align"] = step(f"n {n} K {K} align", align)
            say(sec["align"])

            def pyramid():
                batch, (Tb, sb, stb) = timed(lambda: lib.map_align_pyramid_batch_device(levels, desc, starts, pyr_opts))
                single, Ts = timed(lambda: [lib.map_align_pyramid_device(levels, desc, T, pyr_opts)[0] for T in starts])
                assert not stb.any() and Tb.tobytes() == np.stack(Ts).tobytes()
                return dict(batch=batch, singles=single, speedup=single["ms"] / batch["ms"],
                            rounds=[max(s["iterations"] for s in row) + 1 for row in sb], poses_equal=True)

            sec["pyramid"] = step(f"n {n} K {K} pyramid", pyramid)
            say(sec["pyramid"])
        d.free()
    for m in levels:
        m.close()
    out["complete"] = True
    step("done", dict)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
