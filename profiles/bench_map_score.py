"""Timings of the occupancy score of pose hypotheses (csrc/map.hip: k_map_score_batch) beside the only thing the library
offered for the purpose before it: wc_map_linearize_batch of the same points and poses, whose n_found is a score.  Writes
profiles/map_score_bench.json (--out) after every step, so that a run that does not complete leaves what it measured:
  the map      DESIGN 8.9's room (60 000 points, v = 0.2); its v = 1.6 and v = 0.8 levels are scored
  the scans    g1_room(n, seed + 7), n = 4000 and 48 000, in the sensor frame of tests/map_search_ref.py's true pose
  the poses    wc_pose_grid around tests/map_score_ref.py's start: K = 64 (16 headings x 2 x 2), 1024 (16 x 8 x 8), 7056 (16 x 21 x 21: the
               scene's) and 2^17 (128 x 32 x 32), spaced 0.8 m
  score        PointMap.score_batch_device, min_points 1: the median and minimum of --reps device-timed calls (wc_timer_start /
               wc_timer_stop_ms around the whole call: upload of the poses, kernel, read-back) after one untimed call
  linearize    PointMap.linearize_batch_device of the same points and poses for K <= 1024 (its cap), timed the same way
  check        the timed records' n_in is the scan size for every pose and n_bad is zero
One process; every step runs under its own alarm (--step-limit seconds, default action: the process ends there), and the first step
that fails ends the run.  No figure is a pass condition.
python profiles/bench_map_score.py [--reps 10] [--step-limit 120] [--out profiles/map_score_bench.json]"""
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
import map_score_ref as SC  # noqa: E402
import map_search_ref as MS  # noqa: E402
from map_bench_common import xyz_of  # noqa: E402
from wildcat_slam_amd import lib, synth  # noqa: E402
from wildcat_slam_amd import records as R  # noqa: E402

GRIDS = {64: (16, (2, 2, 1)), 1024: (16, (8, 8, 1)), 7056: (16, (21, 21, 1)), 2**17: (128, (32, 32, 1))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--step-limit", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(HERE, "map_score_bench.json"))
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
        world["levels"] = fine.pyramid(MC.BASIN_FACTOR, MC.BASIN_LEVELS)  # finest first
        return {f"v{m.voxel}": dict(voxels=m.size()[0]) for m in world["levels"]}

    out["maps"] = step("build", build)
    levels = world["levels"]
    scored = {1.6: levels[3], 0.8: levels[2]}
    T_true = MS.search_pose()

    def timed(call):
        ms, res = [], None
        for _ in range(a.reps + 1):
            ctx.sync()
            ctx.timer_start()
            res = call()
            ms.append(ctx.timer_stop_ms())
        return dict(ms=float(np.median(ms[1:])), ms_min=float(np.min(ms[1:]))), res

    poses = {K: lib.pose_grid(SC.scene_start(), n_yaw, n_xyz, SC.SCENE_STEP) for K, (n_yaw, n_xyz) in GRIDS.items()}
    for n in (4000, 48_000):
        p = xyz_of(synth.g1_room(n, seed=synth.SEED + 7)).astype(np.float64)
        scan = ((p - T_true[:, 3]) @ T_true[:, :3]).astype(np.float32)
        d = ctx.to_device(scan)
        desc = R.Points(d.ptr, 0, 12, 0, n)
        for v, m in scored.items():
            prm = lib.map_reg_params(m.voxel)
            for K, Ts in poses.items():
                sec = out.setdefault(f"v{v}_n{n}_K{K}", {})

                def score():
                    t, rec = timed(lambda: m.score_batch_device(desc, Ts, 1))
                    assert np.all(rec["n_in"] == n) and not rec["n_bad"].any()
                    t["ns_per_pair"] = 1e6 * t["ms"] / (K * n)
                    t["best_n_hit"] = int(rec["n_hit"].max())
                    return t

                sec["score"] = step(f"v {v} n {n} K {K} score", score)
                say(sec["score"])
                if K <= 1024:

                    def linearize():
                        t, (ne, status) = timed(lambda: m.linearize_batch_device(desc, Ts, prm))
                        assert not status.any() and ne["n_found"].max() > 0
                        t["ns_per_pair"] = 1e6 * t["ms"] / (K * n)
                        return t

                    sec["linearize_batch"] = step(f"v {v} n {n} K {K} linearize_batch", linearize)
                    sec["linearize_over_score"] = sec["linearize_batch"]["ms"] / sec["score"]["ms"]
                    say(sec["linearize_batch"], "ratio", sec["linearize_over_score"])
        d.free()
    for m in levels:
        m.close()
    out["complete"] = True
    step("done", dict)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
