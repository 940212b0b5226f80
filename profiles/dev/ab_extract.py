"""A/B of the extraction on one box: python profiles/dev/ab_extract.py <tree> [steps] - wall ms per sweep (enqueue + finish) of the C2
sweep as 48-byte records and packed, the firing-order sweep, the 10 M-point cloud in both layouts, with the library of <tree>.
python profiles/dev/ab_extract.py <tree> [steps] exact - the exact path (exact_sums = 1) on the C2 sweep and the firing-order sweep only"""
import os, sys, time
tree = os.path.abspath(sys.argv[1])
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
exact = len(sys.argv) > 3 and sys.argv[3] == "exact"
sys.path.insert(0, os.path.join(tree, "wildcat-slam_amd", "python"))
import numpy as np
from wildcat_slam_amd import lib, synth
from wildcat_slam_amd import records as Rec

ctx = lib.Context(0)
ctx.set_exact_sums(exact)
def run(pts, soa, steps):
    n = len(pts)
    cap = (3 * n) // 20 + 1
    d_out, d_ids = ctx.alloc(cap * 144), ctx.alloc(cap * 16)
    if soa:
        d_xyz = ctx.to_device(np.stack([pts["x"], pts["y"], pts["z"]], axis=1).astype(np.float32).reshape(-1))
        d_t = ctx.to_device(np.ascontiguousarray(pts["time"], np.float64))
        desc = Rec.Points(d_xyz.ptr, d_t.ptr, 12, 8, n)
    else:
        d = ctx.to_device(pts)
        desc = ctx.points_desc(d, n)
    t_lo, t_hi = float(pts["time"][0]), float(pts["time"][-1])
    for _ in range(10):
        ctx.extract_enqueue(desc, d_out, d_ids, cap, t_lo, t_hi)
        m = ctx.extract_finish()
    ctx.sync()
    best = 1e9
    for rep in range(3):
        t0 = time.perf_counter()
        for _ in range(steps):
            ctx.extract_enqueue(desc, d_out, d_ids, cap, t_lo, t_hi)
            m = ctx.extract_finish()
        ctx.sync()
        best = min(best, (time.perf_counter() - t0) / steps)
    ctx.extract_profile(True)
    acc = {}
    for _ in range(20):
        ctx.extract_enqueue(desc, d_out, d_ids, cap, t_lo, t_hi)
        ctx.extract_finish()
        for k, v in ctx.extract_stage_ms().items():
            acc[k] = acc.get(k, 0) + v / 20
    ctx.extract_profile(False)
    return best * 1e3, m, {k: round(v * 1e3, 1) for k, v in acc.items() if k != "init"}

c2 = synth.g2_lattice(3906, m=32)[0]
room = synth.g1_room(1_000_000, seed=synth.SEED + 3)
out = []
work = [("c2", c2, False, steps), ("room", room, False, steps // 2)]
if not exact:
    c5 = synth.g2_lattice(39062, m=32)[0]
    work = [work[0], ("c2soa", c2, True, steps), work[1], ("roomsoa", room, True, steps // 2), ("c5", c5, False, steps // 4), ("c5soa", c5, True, steps // 4)]
for name, pts, soa, st in work:
    ms, m, stg = run(pts, soa, st)
    out.append("%s %.4f %s" % (name, ms, list(stg.values())))
print(os.path.basename(tree) or "new", " | ".join(out))
