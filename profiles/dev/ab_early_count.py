"""A/B of two libraries on ONE box, alternating: python profiles/dev/ab_early_count.py <old tree> <new tree> [alternations] [sweeps] [out.json]
Wall ms per sweep (enqueue + finish, one sync at the end) of a run of `sweeps` sweeps, for the C2 sweep as 48-byte records and packed,
the 1 M-point firing-order sweep, and the 10 M-point cloud in both layouts.  Every alternation starts a fresh process per tree (old, then
new); the clouds are generated once and handed over as .npy files.  Prints and (with out.json) stores min / max / median per workload
and tree, every single run included.
(child: python profiles/dev/ab_early_count.py --child <tree> <cloud dir> <sweeps>)"""
import json, os, statistics, subprocess, sys, tempfile, time

WORK = [("c2_records", "c2", False, 1), ("c2_packed", "c2", True, 1), ("room_1m_firing_order", "room", False, 1),
        ("c5_10m_records", "c5", False, 1), ("c5_10m_packed", "c5", True, 1)]


def child(tree, cloud_dir, sweeps):
    sys.path.insert(0, os.path.join(os.path.abspath(tree), "wildcat-slam_amd", "python"))
    import numpy as np
    from wildcat_slam_amd import lib
    from wildcat_slam_amd import records as Rec

    ctx = lib.Context(0)
    out = {}
    for name, cloud, soa, div in WORK:
        pts = np.load(os.path.join(cloud_dir, cloud + ".npy"))
        n = len(pts)
        cap = (3 * n) // 20 + 1
        d_out, d_ids = ctx.alloc(cap * 144), ctx.alloc(cap * 16)
        if soa:
            d_xyz = ctx.to_device(np.stack([pts["x"], pts["y"], pts["z"]], axis=1).astype(np.float32).reshape(-1))
            d_t = ctx.to_device(np.ascontiguousarray(pts["time"], np.float64))
            keep, desc = (d_xyz, d_t), Rec.Points(d_xyz.ptr, d_t.ptr, 12, 8, n)
        else:
            keep = ctx.to_device(pts)
            desc = ctx.points_desc(keep, n)
        enq, fin = ctx.prepare_extract(desc, d_out, d_ids, cap, float(pts["time"][0]), float(pts["time"][-1]))
        for _ in range(20):
            enq()
            m = fin()
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(sweeps // div):
            enq()
            m = fin()
        ctx.sync()
        out[name] = dict(ms=(time.perf_counter() - t0) / (sweeps // div) * 1e3, surfels=int(m), fast=ctx.extract_path_info()["fast"])
        for b in (d_out, d_ids) + (keep if soa else (keep,)):
            b.free()
    ctx.close()
    print("AB " + json.dumps(out))


def main():
    old, new = sys.argv[1], sys.argv[2]
    alternations = int(sys.argv[3]) if len(sys.argv) > 3 else 6
    sweeps = int(sys.argv[4]) if len(sys.argv) > 4 else 200
    sys.path.insert(0, os.path.join(os.path.abspath(new), "wildcat-slam_amd", "python"))
    import numpy as np
    from wildcat_slam_amd import synth

    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, "c2.npy"), synth.g2_lattice(3906, m=32)[0])
        np.save(os.path.join(d, "room.npy"), synth.g1_room(1_000_000, seed=synth.SEED + 3))
        np.save(os.path.join(d, "c5.npy"), synth.g2_lattice(39062, m=32)[0])
        runs = {"old": [], "new": []}
        for a in range(alternations):
            for which, tree in (("old", old), ("new", new)):
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, d, str(sweeps)], capture_output=True, text=True, timeout=600)
                line = [l for l in p.stdout.splitlines() if l.startswith("AB ")]
                if p.returncode != 0 or not line:
                    sys.exit("child failed (%s, alternation %d, rc %d):\n%s" % (which, a, p.returncode, p.stderr[-2000:]))
                runs[which].append(json.loads(line[0][3:]))
                print(which, a, {k: round(v["ms"], 4) for k, v in runs[which][-1].items()}, flush=True)
    res = {"method": "%d alternations old / new on one box, a fresh process each; ms per sweep (enqueue + finish) over a run of %d sweeps after 20 warm-up sweeps"
                     % (alternations, sweeps), "workloads": {}}
    for name, *_ in WORK:
        w = {}
        for which in ("old", "new"):
            ms = [r[name]["ms"] for r in runs[which]]
            w[which] = dict(min=round(min(ms), 5), max=round(max(ms), 5), median=round(statistics.median(ms), 5), runs=[round(x, 5) for x in ms],
                            surfels=runs[which][0][name]["surfels"], default_path=all(r[name]["fast"] for r in runs[which]))
        w["ranges_apart"] = w["new"]["max"] < w["old"]["min"]
        w["new_median_at_or_below_old_max"] = w["new"]["median"] <= w["old"]["max"]
        res["workloads"][name] = w
    print(json.dumps(res, indent=1))
    if len(sys.argv) > 5:
        json.dump(res, open(sys.argv[5], "w"), indent=1)
        open(sys.argv[5], "a").write("\n")


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    else:
        main()
