"""Timings of the removal in place (csrc/map.hip: k_map_erase, k_map_remove_keys) beside the counting wc_map_carve.  Writes
profiles/map_remove_bench.json (--out) after every step, so that a run that does not complete leaves what it measured:
  the map          ONE one-million-point room sweep (synth.g1_room) inserted once into a map created with reserve_voxels = 2^20, v = 0.2:
                   no growth, no clear, no crop; a second sweep of that room supplies the rays (1 M, max_range 30 m, shell 1, min_rays 2)
  carve_ms         wc_map_carve, median and minimum of --reps device-timed calls (wc_timer_start / wc_timer_stop_ms around the whole call)
  remove_first_ms  the first wc_map_carve_remove: ONE call - it cannot be repeated on the same map
  remove_again_ms  wc_map_carve_remove on the already carved map (it selects nothing): median and minimum of --reps calls
  remove_keys_ms   wc_map_remove_keys of the set the first call removed, on fresh copies of the uncarved map, each built by wc_map_absorb
                   of its state into a new map created with reserve_voxels = 2^20: one call per copy, median and minimum of --reps copies
  facade           Odometry.map_ms() per sweep (median, maximum) on the stream of tests/test_map_remove_gpu.py::test_facade with
                   set_map_carve off and on (12 m, shell 1, min_rays 1)
One process; every step runs under its own alarm (--step-limit seconds, default action: the process ends there).
python profiles/bench_map_remove.py [--reps 5] [--step-limit 60] [--out profiles/map_remove_bench.json]"""
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

from wildcat_slam_amd import lib, synth  # noqa: E402
from wildcat_slam_amd import records as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-limit", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(HERE, "map_remove_bench.json"))
    a = ap.parse_args()
    out = dict(reps=a.reps, max_range=30.0, shell=1, min_rays=2, voxel=0.2, complete=False, steps_done=[])
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
    n_sweep, v = 1_000_000, 0.2
    sweep, rays = step("sweeps", lambda: (synth.g1_room(n_sweep, seed=200, t_start=1000.0), synth.g1_room(n_sweep, seed=300, t_start=1005.5)))
    origin = synth.traj_pos(0.25) + np.array([0.0, 0.0, 1.5])
    d_sweep, d_rays = ctx.to_device(sweep), ctx.to_device(rays)
    sweep_desc = R.Points(d_sweep.ptr, d_sweep.ptr + 24, 48, 48, len(sweep))
    ray_desc = R.Points(d_rays.ptr, 0, 48, 0, len(rays))
    params = lib.map_carve_params(30.0, 0.0, 1, 2, 4096)
    m = ctx.map_create(v, reserve_voxels=1 << 20)
    sec = out.setdefault("map_calls", {})

    def build():
        ctx._ck(ctx.lib.wc_map_insert(ctx.h, m.h, C.byref(sweep_desc), None))
        voxels, info = m.size()[0], m.info()
        say("map built:", voxels, "voxels,", info["slots"], "slots,", info["growths"], "growths")
        return dict(voxels=voxels, slots=info["slots"], growths=info["growths"])

    def timed(call, reps, label):
        ms, res = [], None
        for rep in range(reps):
            ctx.timer_start()
            res = call()
            ms.append(ctx.timer_stop_ms())
            say(label, "rep", rep, "%.3f ms" % ms[-1])
        return ms, res

    def carve():
        ms, res = timed(lambda: m.carve_device(ray_desc, origin, params), a.reps + 1, "carve")  # (the first call takes the scratch: not timed)
        return dict(carve_ms=float(np.median(ms[1:])), carve_ms_min=float(np.min(ms[1:])), steps=res["steps"], rays_used=res["rays_used"],
                    voxels_selected=res["voxels_removed"], points_selected=res["points_removed"])

    state = {}

    def remove_first():
        state["vox"], _ = m.state()
        ms, res = timed(lambda: m.carve_remove_device(ray_desc, origin, params), 1, "carve_remove (first)")
        info = m.info()
        return dict(remove_first_ms=ms[0], voxels_removed=res["voxels_removed"], points_removed=res["points_removed"], voxels_left=m.size()[0],
                    tombstones=m.tombstones()[0], slots=info["slots"], growths=info["growths"])

    def remove_again():
        ms, res = timed(lambda: m.carve_remove_device(ray_desc, origin, params), a.reps, "carve_remove (again)")
        return dict(remove_again_ms=float(np.median(ms)), remove_again_ms_min=float(np.min(ms)), voxels_removed_again=res["voxels_removed"])

    def remove_keys():
        left = m.export()[2]
        was = state["vox"]["key"]
        pack = lambda k: ((k[:, 0].astype(np.int64) + 2**20) << 42) | ((k[:, 1].astype(np.int64) + 2**20) << 21) | (k[:, 2].astype(np.int64) + 2**20)  # noqa: E731
        gone = np.ascontiguousarray(was[~np.isin(pack(was), pack(left))], np.int32)
        d_keys = ctx.to_device(gone)
        ms, res = [], None
        for rep in range(a.reps):
            c = ctx.map_create(v, reserve_voxels=1 << 20)
            assert c.absorb(state["vox"]) == 0
            ctx.timer_start()
            res = c.remove_device(d_keys, len(gone))
            ms.append(ctx.timer_stop_ms())
            say("remove_keys rep", rep, "%.3f ms" % ms[-1], res, c.info()["slots"], "slots")
            c.close()
        d_keys.free()
        return dict(remove_keys_ms=float(np.median(ms)), remove_keys_ms_min=float(np.min(ms)), keys=len(gone), **res)

    sec["map"] = step("build", build)
    step("carve", carve, sec)
    step("carve_remove first", remove_first, sec)
    step("carve_remove again", remove_again, sec)
    step("remove_keys", remove_keys, sec)
    m.close()

    def facade(on):
        from test_map_gpu import _drive

        msgs, imu, _ = synth.raw_stream(1.7, pts_per_s=300_000, gyro_bias=(0.0, 0.0, 0.02), t_start=1000.0)
        odo = lib.Odometry(0)
        odo.set_fill_outputs(True)
        odo.set_map_voxel(0.5)
        if on:
            odo.set_map_carve(12.0, 1, 1)
        ms = []
        _drive(odo, msgs, imu, lambda: ms.append(odo.map_ms()))
        voxels = odo.map_size()[0]
        odo.close()
        return {("on" if on else "off"): dict(sweeps=len(ms), map_ms_median=float(np.median(ms)), map_ms_max=float(np.max(ms)), voxels=voxels)}

    fac = out.setdefault("facade", {})
    step("facade off", lambda: facade(False), fac)
    step("facade on", lambda: facade(True), fac)
    out["complete"] = True
    step("done", dict)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
