"""Timings of a map merged under a rigid pose (csrc/map.hip: k_map_merge_moved) beside a wc_map_merge of the same source.
Writes profiles/map_moved_bench.json (--out) after every step, so that a run that does not complete leaves what it measured:
  the map       the 11 one-million-point room sweeps of profiles/bench_map_surfels.py inserted into a moments map, at v = 0.05 and 0.2
  merge_moved   wc_map_merge_moved of that map under a pose of 10 degrees about (1, 2, 3) and (0.37, -1.2, 0.05) m into a destination created
                inside the timer with reserve_voxels = 0, with moments and plain, h_out = NULL: the whole call - the size read-back, the
                growth of the empty table, the kernel - device-timed; the destination is destroyed outside the timer
  merge         wc_map_merge of the same map into the same kind of destination: the same pass over the source's slots and the same table to
                make, no arithmetic and no two lanes on one voxel.  Its kernel is not touched by this feature: the yardstick
                each the median and minimum of --reps device-timed calls (wc_timer_start / wc_timer_stop_ms around the whole call) after
                --warmup untimed calls; per_voxel_ns = the median over the SOURCE's voxels
  check         what was timed is what the tests check: 3000 voxels of the v = 0.2 map moved on the device against tests/map_moved_ref.py
One process; every step runs under its own alarm (--step-limit seconds, default action: the process ends there), and the first step
that fails ends the run.
python profiles/bench_map_moved.py [--reps 20] [--warmup 3] [--step-limit 120] [--out profiles/map_moved_bench.json]"""
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

import map_moved_ref as MM  # noqa: E402
from wildcat_slam_amd import lib, synth  # noqa: E402
from wildcat_slam_amd import records as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-limit", type=int, default=120)
    ap.add_argument("--sweeps", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(HERE, "map_moved_bench.json"))
    a = ap.parse_args()
    out = dict(reps=a.reps, warmup=a.warmup, sweeps=a.sweeps, complete=False, steps_done=[])
    t_start = time.perf_counter()
    T = MM.pose_of(10.0, (1.0, 2.0, 3.0), (0.37, -1.2, 0.05))

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
        """warm-ups, then `reps` device-timed calls; call() -> the map it made, closed outside the timer"""
        ms = []
        for _ in range(a.warmup + a.reps):
            ctx.sync()
            ctx.timer_start()
            made = call()
            ms.append(ctx.timer_stop_ms())
            made.close()
        ms = ms[a.warmup:]
        med = float(np.median(ms))
        return dict(ms=med, ms_min=float(np.min(ms)), per_voxel_ns=med * 1e6 / n_vox)

    for v, m in maps.items():
        sec = out.setdefault(f"v{v}", {})
        n = out["maps"][f"v{v}"]["voxels"]
        for moments in (True, False):
            kind = "moments" if moments else "plain"

            def merge():
                t = ctx.map_create(v, moments=moments)
                t.merge(m)
                return t

            def merge_moved():
                t = ctx.map_create(v, moments=moments)
                t.merge_moved(m, T, want_counts=False)
                return t

            sec[f"merge_{kind}"] = step(f"v{v} merge {kind}", lambda: timed(merge, n))
            res = step(f"v{v} merge_moved {kind}", lambda: timed(merge_moved, n))
            t = ctx.map_create(v, moments=moments)
            res["counts"] = t.merge_moved(m, T)
            res["voxels_out"], res["slots_out"] = t.size()[0], t.info()["slots"]
            res["over_merge"] = res["ms"] / sec[f"merge_{kind}"]["ms"]
            t.close()
            sec[f"merge_moved_{kind}"] = res
            say(f"v{v} {kind}:", res, "merge:", sec[f"merge_{kind}"])

    def check():
        v = 0.2
        vox, mom = maps[v].state()
        vox, mom = vox[:3000], mom[:3000]
        src = ctx.map_create(v, moments=True)
        src.absorb(vox, mom)
        moved = src.moved(T)
        got = moved.state()
        want = MM.merge_moved_ref((vox[:0], mom[:0]), (vox, mom), v, T)
        ok = len(vox) == 3000 and got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        src.close(), moved.close()
        assert ok
        return dict(voxels=len(vox), voxels_out=len(got[0]), state_equal=ok)

    out["check"] = step("check", check)
    for m in maps.values():
        m.close()
    out["complete"] = True
    step("done", dict)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
