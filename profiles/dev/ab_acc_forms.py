"""A/B of k_fx_acc's forms (development option fx_acc_form) in ONE process on the same device-resident sweep:
python profiles/dev/ab_acc_forms.py [c2|c2soa|room|c5] [alternations] [sweeps] [out.json]
alternates the forms 0 / 1 / 2 / -1 (the library's own) and prints, per form, the wall ms per sweep (enqueue + finish) of every
alternation and the k_fx_acc<1> and k_fx_nodes<1> times from the stage events (us, a profiled run of its own)."""
import json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "wildcat-slam_amd", "python"))
import numpy as np
from wildcat_slam_amd import lib, synth
from wildcat_slam_amd import records as Rec

which = sys.argv[1] if len(sys.argv) > 1 else "c2"
alts = int(sys.argv[2]) if len(sys.argv) > 2 else 5
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 200
out = sys.argv[4] if len(sys.argv) > 4 else None
pts = {"c2": lambda: synth.g2_lattice(3906, m=32)[0], "c2soa": lambda: synth.g2_lattice(3906, m=32)[0], "c5": lambda: synth.g2_lattice(39062, m=32)[0],
       "room": lambda: synth.g1_room(1_000_000, seed=synth.SEED + 3)}[which]()
n = len(pts)
cap = (3 * n) // 20 + 1
ctx = lib.Context(0)
d_out, d_ids = ctx.alloc(cap * 144), ctx.alloc(cap * 16)
if which.endswith("soa"):
    d_xyz = ctx.to_device(np.stack([pts["x"], pts["y"], pts["z"]], axis=1).astype(np.float32).reshape(-1))
    d_t = ctx.to_device(np.ascontiguousarray(pts["time"], np.float64))
    desc = Rec.Points(d_xyz.ptr, d_t.ptr, 12, 8, n)
else:
    d = ctx.to_device(pts)
    desc = ctx.points_desc(d, n)
t_lo, t_hi = float(pts["time"][0]), float(pts["time"][-1])
enqueue, finish = ctx.prepare_extract(desc, d_out, d_ids, cap, t_lo, t_hi)
FORMS = (0, 1, 2, -1)
wall = {f: [] for f in FORMS}
acc = {f: [] for f in FORMS}
nodes = {f: [] for f in FORMS}
for a in range(alts):
    for f in FORMS:
        ctx.set_dev_option("fx_acc_form", f)
        for _ in range(20):
            enqueue(), finish()
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            enqueue(), finish()
        ctx.sync()
        wall[f].append(round((time.perf_counter() - t0) / steps * 1e3, 5))
        ctx.extract_profile(True)
        v, w = [], []
        for _ in range(24):
            enqueue(), finish()
            st = ctx.extract_stage_ms()
            v.append(st["point_sort"]), w.append(st["roots_stream"])
        ctx.extract_profile(False)
        acc[f].append(round(1e3 * float(np.median(v[4:])), 2))
        nodes[f].append(round(1e3 * float(np.median(w[4:])), 2))
res = dict(workload=which, points=n, alternations=alts, sweeps=steps, assert_fast=ctx.extract_path_info()["fast"],
           wall_ms={str(f): wall[f] for f in FORMS}, k_fx_acc_us={str(f): acc[f] for f in FORMS}, k_fx_nodes_us={str(f): nodes[f] for f in FORMS})
for f in FORMS:
    print("form %2d: wall ms %s  [%.5f .. %.5f]   k_fx_acc us %s   k_fx_nodes us %s" % (f, wall[f], min(wall[f]), max(wall[f]), acc[f], nodes[f]))
print(json.dumps(res))
if out:
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
ctx.close()
