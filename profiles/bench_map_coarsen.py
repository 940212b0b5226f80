"""Timings of the voxel map's coarser levels (csrc/map.hip: k_map_coarsen) beside a wc_map_merge of the same source.
Writes profiles/map_coarsen_bench.json (--out) after every step, so that a run that does not complete leaves what it measured:
  the map      the 11 one-million-point room sweeps of profiles/bench_map.py inserted into a moments map, at v = 0.05 and 0.2
  coarsen      wc_map_coarsen(factor) of that map, factor 2 and 4, with moments and (flags 0) plain: the whole call - the size read-back,
               the new table and its clearing, the kernel - device-timed; the result is destroyed outside the timer.  Factor 1 beside
               them: the same call and kernel with every voxel on a slot of its own (a copy), the figure without two lanes on one voxel
  merge        wc_map_merge of the same map into an empty map created with reserve_voxels = 0 (with moments, and plain): the same pass over
               the source's slots, the same table to make, no re-basing and no two lanes on one voxel
               each the median and minimum of --reps device-timed calls (wc_timer_start / wc_timer_stop_ms around the whole call) after
               one untimed call; per_voxel_ns = the median over the SOURCE's voxels
  check        what was timed is what the tests check: the v = 0.2 map's coarsened state (factor 2) against tests/map_coarsen_ref.py
  facade       a 1.7 s room stream through LidarOdometry (v = 0.1, map_surfels on), then one RelocalizeToMap (factor 2, 3 levels) against
               one AlignToMap of the same scan from the same pose: wall time, the median of --reps calls each; and the rebuild of the two
               coarser levels alone (PointMap.pyramid on a stand-alone map of the same sweeps), device-timed
One process; every step runs under its own alarm (--step-limit seconds, default action: the process ends there), and the first step
that fails ends the run.
python profiles/bench_map_coarsen.py [--reps 20] [--step-limit 120] [--out profiles/map_coarsen_bench.json]"""
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

import map_coarsen_ref as MC  # noqa: E402
from map_bench_common import xyz_of  # noqa: E402
from wildcat_slam_amd import lib, synth  # noqa: E402
from wildcat_slam_amd import records as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-limit", type=int, default=120)
    ap.add_argument("--sweeps", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(HERE, "map_coarsen_bench.json"))
    a = ap.parse_args()
    out = dict(reps=a.reps, sweeps=a.sweeps, complete=False, steps_done=[])
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
    maps = {v: ctx.map_create(v, moments=True) for v in (0.05, 0.2)}

    def build():
        for i in range(a.sweeps):
            sweep = synth.g1_room(n_sweep, seed=200 + i, t_start=1000.0 + 0.5 * i)
            d = ctx.to_device(sweep)
            desc = R.Points(d.ptr, d.ptr + 24, 48, 48, len(sweep))
            for m in maps.values():
                ctx._ck(ctx.lib.wc_map_insert(ctx.h, m.h, C.byref(desc), None))
            ctx.sync()
            d.free()
        return {f"v{v}": dict(voxels=m.size()[0], points=m.size()[1], slots=m.info()["slots"]) for v, m in maps.items()}

    out["maps"] = step("build", build)

    def timed(call, n_vox):
        """`reps` + 1 device-timed calls, the first not counted; call() -> the map it made, closed outside the timer"""
        ms = []
        for _ in range(a.reps + 1):
            ctx.sync()
            ctx.timer_start()
            made = call()
            ms.append(ctx.timer_stop_ms())
            made.close()
        med = float(np.median(ms[1:]))
        return dict(ms=med, ms_min=float(np.min(ms[1:])), per_voxel_ns=med * 1e6 / n_vox)

    for v, m in maps.items():
        sec = out.setdefault(f"v{v}", {})
        n = out["maps"][f"v{v}"]["voxels"]
        for moments in (True, False):
            kind = "moments" if moments else "plain"

            def merge():
                t = ctx.map_create(v, moments=moments)
                t.merge(m)
                return t

            sec[f"merge_{kind}"] = step(f"v{v} merge {kind}", lambda: timed(merge, n))
            for factor in (1, 2, 4):

                def coarsen():
                    c = m.coarsen(factor, moments)
                    return c

                res = step(f"v{v} coarsen x{factor} {kind}", lambda: timed(coarsen, n))
                c = m.coarsen(factor, moments)
                res["voxels_out"], res["slots_out"] = c.size()[0], c.info()["slots"]
                res["over_merge"] = res["ms"] / sec[f"merge_{kind}"]["ms"]
                c.close()
                sec[f"coarsen_x{factor}_{kind}"] = res
                say(f"v{v} x{factor} {kind}:", res)

    def check():
        v = 0.2
        vox, mom = maps[v].state()
        c = maps[v].coarsen(2)
        got = c.state()
        want = MC.coarsen_ref(vox, mom, v, 2)
        ok = len(vox) > 0 and got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        c.close()
        assert ok
        return dict(voxels=len(vox), voxels_out=len(got[0]), state_equal=ok)

    out["check"] = step("check", check)
    for m in maps.values():
        m.close()

    def facade():
        from test_map_gpu import _drive

        msgs, imu, _ = synth.raw_stream(1.7, pts_per_s=300_000, gyro_bias=(0.0, 0.0, 0.02), t_start=1000.0)
        odo = lib.Odometry(0)
        odo.set_fill_outputs(True)
        odo.set_map_voxel(0.1)
        odo.set_map_surfels(True)
        scans = []
        _drive(odo, msgs, imu, lambda: scans.append(xyz_of(odo.outputs()["scan"])))
        q = scans[-1][::3]
        T = np.eye(3, 4)
        T[:, 3] = [0.1, -0.2, 0.05]
        opts = lib.map_align_opts(lib.map_reg_params(0.2, 3, cauchy_a=0.4), max_iterations=6)
        wall = dict(relocalize=[], align=[])
        res = {}
        for _ in range(a.reps + 1):
            for name, call in (("relocalize", lambda: odo.map_relocalize(q, T, 2, 3, opts)), ("align", lambda: odo.map_align(q, T, opts))):
                t0 = time.perf_counter()
                res[name] = call()
                wall[name].append((time.perf_counter() - t0) * 1e3)
        iters = dict(relocalize=[s["iterations"] for s in res["relocalize"][1]], align=[res["align"][1]["iterations"]])
        r = dict(voxels=odo.map_size()[0], scan_points=len(q), iterations=iters)
        for name, ms in wall.items():
            r[f"{name}_wall_ms"], r[f"{name}_wall_ms_min"] = float(np.median(ms[1:])), float(np.min(ms[1:]))
        odo.close()
        # the rebuild alone: the two coarser levels of a stand-alone map of the same sweeps, device-timed
        ref = ctx.map_create(0.1, moments=True)
        for s in scans:
            ref.insert(s)
        ms = []
        for _ in range(a.reps + 1):
            ctx.sync()
            ctx.timer_start()
            levels = ref.pyramid(2, 3)
            ms.append(ctx.timer_stop_ms())
            for m in levels[1:]:
                m.close()
        ref.close()
        r["levels_rebuild_ms"], r["levels_rebuild_ms_min"] = float(np.median(ms[1:])), float(np.min(ms[1:]))
        return r

    out["facade"] = step("facade", facade)
    out["complete"] = True
    step("done", dict)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
