"""What the bench_map*.py scripts share: progress notes, the device-timed repetition loop and the packed coordinates of POINT records."""
import sys
import time

import numpy as np

T0 = time.perf_counter()


def note(*what):
    """progress on stderr (stdout carries the JSON object alone)"""
    print("[%7.1f s]" % (time.perf_counter() - T0), *what, file=sys.stderr, flush=True)


def timed(ctx, fn, reps, warmup=3):
    """fn(timer): runs its untimed preparation, starts the timer (ctx.timer_start) when `timer` is true, runs the timed call
    -> median and minimum [ms] of `reps` device-timed calls after `warmup` untimed ones"""
    for _ in range(warmup):
        fn(False)
        ctx.sync()
    out = []
    for _ in range(reps):
        fn(True)
        out.append(ctx.timer_stop_ms())
    return dict(median=float(np.median(out)), min=float(np.min(out)))


def xyz_of(p):
    """POINT records -> their packed (n, 3) float32 coordinates"""
    return np.stack([p["x"], p["y"], p["z"]], -1).astype(np.float32)
