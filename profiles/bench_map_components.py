"""Timings of wc_map_components and wc_map_remove_small (csrc/map.hip: k_map_cc_*) beside wc_map_export, which pays the same
compaction and sort.  Writes profiles/map_components_bench.json (--out) after every step, so that a run that does not complete leaves what
it measured:
  the map        ONE one-million-point room sweep (synth.g1_room) inserted once into a map created with reserve_voxels = 2^20, at v = 0.2
                 and 0.05: no growth, no clear, no crop, no second insert
  components_ms  wc_map_components (keys, labels and records written) at connectivity 6, 18 and 26, min_points 1; median and minimum of
                 --reps device-timed calls (wc_timer_start / wc_timer_stop_ms around the whole call, its two read-backs included)
  export_ms      wc_map_export of the same map, the same way
  remove_ms      wc_map_remove_small (min_voxels 5, connectivity 26) on fresh copies of the map, each built by wc_map_absorb of the map's
                 state into a reserved map (the copy is not timed); one timed call per copy, --reps copies
  cpu            wc_map_label_keys on the same export at connectivity 26, wall time, and - where it imports - scipy.ndimage.label with the
                 full structuring element on the dense grid of the export's bounding box (skipped, and said so, above 2^28 cells)
One process; every step runs under its own alarm (--step-limit seconds, default action: the process ends there).
python profiles/bench_map_components.py [--reps 5] [--step-limit 60] [--out profiles/map_components_bench.json]"""
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
    ap.add_argument("--out", default=os.path.join(HERE, "map_components_bench.json"))
    a = ap.parse_args()
    out = dict(reps=a.reps, complete=False, steps_done=[])
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
    sweep = step("sweep", lambda: synth.g1_room(n_sweep, seed=200, t_start=1000.0))
    d_sweep = ctx.to_device(sweep)
    sweep_desc = R.Points(d_sweep.ptr, d_sweep.ptr + 24, 48, 48, len(sweep))
    out["points_per_sweep"] = len(sweep)
    for v in (0.2, 0.05):
        m = ctx.map_create(v, reserve_voxels=1 << 20)
        sec = out.setdefault(f"v{v}", {})

        def build():
            ctx._ck(ctx.lib.wc_map_insert(ctx.h, m.h, C.byref(sweep_desc), None))
            voxels, info = m.size()[0], m.info()
            say("map built:", voxels, "voxels,", info["slots"], "slots,", info["growths"], "growths")
            return dict(voxels=voxels, slots=info["slots"], growths=info["growths"])

        sec["map"] = step(f"v{v} build", build)
        n = sec["map"]["voxels"]
        d_keys, d_label, d_comps = ctx.alloc(12 * n), ctx.alloc(4 * n), ctx.alloc(40 * n)
        d_xyz, d_count = ctx.alloc(12 * n), ctx.alloc(4 * n)

        def components(conn):
            p = lib.map_cc_params(conn, 1)
            ms, res = [], None
            for rep in range(a.reps + 1):  # (the first call takes the scratch: not timed)
                ctx.timer_start()
                rc, res = m.components_device(p, d_keys, d_label, n, d_comps, n)
                ms.append(ctx.timer_stop_ms())
                ctx._ck(rc)
                say("components", conn, "rep", rep, "%.3f ms" % ms[-1])
            med = float(np.median(ms[1:]))
            return {f"conn_{conn}": dict(components_ms=med, components_ms_min=float(np.min(ms[1:])), voxels_per_s=n / (med * 1e-3), **res)}

        def export():
            ms = []
            for rep in range(a.reps + 1):
                ctx.timer_start()
                rc, _ = m.export_device(d_xyz, d_count, d_keys, n)
                ctx.sync()
                ms.append(ctx.timer_stop_ms())
                ctx._ck(rc)
                say("export rep", rep, "%.3f ms" % ms[-1])
            return dict(export_ms=float(np.median(ms[1:])), export_ms_min=float(np.min(ms[1:])))

        for conn in (6, 18, 26):
            step(f"v{v} components {conn}", lambda: components(conn), sec)
        step(f"v{v} export", export, sec)

        def remove():
            vox, _ = m.state()
            d_vox = ctx.to_device(vox)
            ms, res = [], None
            for rep in range(a.reps + 1):  # (the first copy's call takes that copy's scratch like every other copy's: all are alike, the first is dropped all the same)
                c = ctx.map_create(v, reserve_voxels=1 << 20)
                c.absorb_device(d_vox, None, len(vox))
                ctx.timer_start()
                res = c.remove_small(5, 0, 26, 1)
                ms.append(ctx.timer_stop_ms())
                say("remove_small rep", rep, "%.3f ms" % ms[-1], res)
                c.close()
            d_vox.free()
            return dict(remove_ms=float(np.median(ms[1:])), remove_ms_min=float(np.min(ms[1:])), min_voxels=5, **res)

        step(f"v{v} remove_small", remove, sec)

        def cpu():
            _, cnt, keys = m.export()
            t0 = time.perf_counter()
            _, _, res = lib.map_label_keys(keys, cnt, 26, 1)
            got = dict(label_keys_s=time.perf_counter() - t0, label_keys=res)
            try:
                from scipy import ndimage
            except ImportError:
                got["scipy"] = "not installed"
                return got
            lo = keys.min(0)
            shape = tuple(int(x) for x in keys.max(0) - lo + 1)
            if np.prod([float(x) for x in shape]) > 2**28:
                got["scipy"] = "skipped: a dense grid of %d x %d x %d cells" % shape
                return got
            t0 = time.perf_counter()
            grid = np.zeros(shape, bool)
            grid[tuple((keys - lo).T)] = True
            _, n_comp = ndimage.label(grid, structure=np.ones((3, 3, 3), bool))
            got.update(scipy_label_s=time.perf_counter() - t0, scipy_components=int(n_comp), scipy_grid=list(shape))
            return got

        sec["cpu"] = step(f"v{v} cpu", cpu)
        for b in (d_keys, d_label, d_comps, d_xyz, d_count):
            b.free()
        m.close()
    out["complete"] = True
    step("done", dict)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
