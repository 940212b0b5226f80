"""Timings of the voxel map's exact state (csrc/map.hip: k_map_state, k_map_absorb, k_map_merge) beside the wc_map_insert
that built the map.  Writes profiles/map_state_bench.json (--out) after every step, so that a run that does not complete leaves what
it measured:
  the map      ONE one-million-point room sweep (synth.g1_room) inserted into a map created with reserve_voxels = 2^20, at v = 0.2 and
               0.05, plain and with moments: no growth, no clear, no crop
  insert_ms    wc_map_insert of that sweep into a fresh reserved map (created outside the timer)
  export_ms    wc_map_export_state of the built map (size read-back, compaction, sort, k_map_state)
  absorb_ms    wc_map_absorb of that state, already in HBM, into a fresh reserved map
  merge_ms     wc_map_merge of the built map into a fresh reserved map
               each the median and minimum of --reps device-timed calls (wc_timer_start / wc_timer_stop_ms around the whole call) after
               one untimed call; per_voxel_ns = the median over the map's voxels.  The insert's kernels are the ones every earlier
               version of the map has (this feature does not touch them), so absorb and merge per voxel against the insert of the same
               sweep compare within one run
  cpu          the numpy restatement: the state of the sweep (tests/map_state_ref.state_of) and two half states added up by key, wall time
One process; every step runs under its own alarm (--step-limit seconds, default action: the process ends there), and the first step
that fails ends the run.
python profiles/bench_map_state.py [--reps 20] [--step-limit 120] [--out profiles/map_state_bench.json]"""
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

import map_query_ref as Q  # noqa: E402
import map_state_ref as MS  # noqa: E402
from map_bench_common import xyz_of  # noqa: E402
from wildcat_slam_amd import lib, synth  # noqa: E402
from wildcat_slam_amd import records as R  # noqa: E402

RESERVE = 1 << 20


def add_by_key(states):
    """states added up by key with numpy alone (no rejected record among them): what absorb_ref does record by record"""
    vox = np.concatenate([s[0] for s in states])
    words = np.concatenate([np.concatenate([s[0]["count"].astype(np.int64)[:, None], s[0]["sum"], s[1]], axis=1) for s in states])
    packed = Q.pack(vox["key"].astype(np.int64))
    order = np.argsort(packed, kind="stable")
    _, start = np.unique(packed[order], return_index=True)
    return vox["key"][order][start], np.add.reduceat(words[order], start, axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-limit", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(HERE, "map_state_bench.json"))
    a = ap.parse_args()
    out = dict(reps=a.reps, reserve_voxels=RESERVE, complete=False, steps_done=[])
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
    sweep = step("sweep", lambda: synth.g1_room(1_000_000, seed=200, t_start=1000.0))
    xyz = xyz_of(sweep)
    d_sweep = ctx.to_device(sweep)
    desc = R.Points(d_sweep.ptr, d_sweep.ptr + 24, 48, 48, len(sweep))
    out["points_per_sweep"] = len(sweep)

    def timed(prepare, call, n_vox):
        """`reps` + 1 times: prepare() outside the timer -> what call() works on; the first call is not counted"""
        ms = []
        for _ in range(a.reps + 1):
            target = prepare()
            ctx.sync()
            ctx.timer_start()
            call(target)
            ms.append(ctx.timer_stop_ms())
            if target is not None:
                target.close()
        med = float(np.median(ms[1:]))
        return dict(ms=med, ms_min=float(np.min(ms[1:])), per_voxel_ns=med * 1e6 / n_vox)

    for v in (0.2, 0.05):
        for moments in (False, True):
            name = f"v{v}_{'moments' if moments else 'plain'}"
            sec = out.setdefault(name, {})
            fresh = lambda: ctx.map_create(v, reserve_voxels=RESERVE, moments=moments)  # noqa: E731
            m = fresh()

            def build():
                ctx._ck(ctx.lib.wc_map_insert(ctx.h, m.h, C.byref(desc), None))
                voxels, info = m.size()[0], m.info()
                say(name, "built:", voxels, "voxels,", info["slots"], "slots,", info["growths"], "growths")
                assert info["growths"] == 0
                return dict(voxels=voxels, slots=info["slots"], growths=info["growths"], record_bytes=112 if moments else 40)

            sec["map"] = step(f"{name} build", build)
            n = sec["map"]["voxels"]
            d_vox, d_mom = ctx.alloc(40 * n), (ctx.alloc(72 * n) if moments else None)
            insert = lambda t: ctx._ck(ctx.lib.wc_map_insert(ctx.h, t.h, C.byref(desc), None))  # noqa: E731
            sec["insert"] = step(f"{name} insert", lambda: timed(fresh, insert, n))

            def export(_):
                rc, got = m.state_device(d_vox, d_mom, n)
                ctx._ck(rc)
                assert got == n

            sec["export_state"] = step(f"{name} export_state", lambda: timed(lambda: None, export, n))
            sec["absorb"] = step(f"{name} absorb", lambda: timed(fresh, lambda t: t.absorb_device(d_vox, d_mom, n, want_count=False), n))
            sec["merge"] = step(f"{name} merge", lambda: timed(fresh, lambda t: t.merge(m), n))

            def check():
                """what was timed is what the tests check: the absorbed and the merged map have the built map's state"""
                want = [x.tobytes() for x in m.state() if x is not None]
                for how in ("absorb", "merge"):
                    t = fresh()
                    if how == "absorb":
                        assert t.absorb_device(d_vox, d_mom, n) == 0
                    else:
                        t.merge(m)
                    assert [x.tobytes() for x in t.state() if x is not None] == want and t.info()["growths"] == 0, how
                    t.close()
                return dict(state_equal=True)

            sec["check"] = step(f"{name} check", check)
            for b in (d_vox, d_mom):
                if b:
                    b.free()
            m.close()

        def cpu():
            t0 = time.perf_counter()
            whole = MS.state_of(xyz, v)
            t1 = time.perf_counter()
            halves = [MS.state_of(xyz[0::2], v), MS.state_of(xyz[1::2], v)]
            t2 = time.perf_counter()
            keys, words = add_by_key(halves)
            t3 = time.perf_counter()
            assert np.array_equal(keys, whole[0]["key"]) and np.array_equal(words[:, 1:4], whole[0]["sum"]) and np.array_equal(words[:, 4:], whole[1])
            return dict(voxels=len(keys), state_of_seconds=t1 - t0, add_by_key_seconds=t3 - t2, add_by_key_records=sum(len(h[0]) for h in halves))

        out[f"v{v}_cpu_numpy"] = step(f"v{v} cpu", cpu)
    out["complete"] = True
    step("done", dict)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
