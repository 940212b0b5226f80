"""A/B of the LM loop's host side (csrc/lm_loop.h): the figures a host decision between two iterations' launches could move.
python profiles/dev/ab_lm_loop.py run [TREE]      one fresh process on TREE's library (default: this tree; e.g. ab_old) -> one JSON line:
    lm_iters_per_s, solve_ms     the bench's C4 window (20 x 50 000 surfels) as bench_window times it - one untimed solve, then a timed one -
                                 repeated five times in the process, the median
    step_solve_ms                the odometry step's solve stage (10 x C2 window, StepWindow), median of 7 steps
    facade_ms_per_lm_iteration   bench.py's bench_facade_stream: ms_per_lm_iteration_median
python profiles/dev/ab_lm_loop.py summarize RUNS.jsonl   lines of `run` tagged {"side": "parent" | "branch"} -> min / median / max per
    side and figure, and the bar: the branch's median no worse than the parent's by more than the parent's own max - min
profiles/dev/ab_lm_loop.sh alternates the two trees."""
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
HIGHER_IS_BETTER = {"lm_iters_per_s"}


def run(tree):
    sys.path[:0] = [os.path.join(tree, "wildcat-slam_amd", "python"), tree]
    import numpy as np

    import bench
    from wildcat_slam_amd import lib, synth
    from wildcat_slam_amd.step import StepWindow

    assert os.path.samefile(os.path.dirname(lib.so_path()), os.path.join(tree, "wildcat-slam_amd", "csrc"))
    ctx = lib.Context(0)
    w = synth.surfel_window(20, 50000, seed=synth.SEED + 7, fixed_patches=50000)
    n_s = len(w["surf"])
    d_surf, d_pose = ctx.to_device(w["surf"]), ctx.to_device(w["pose"])
    d_fs, d_fp = ctx.to_device(w["fix_surf"]), ctx.to_device(w["fix_pose"])
    d_pairs, d_pf = ctx.alloc(8 * n_s), ctx.alloc(8 * n_s)
    n_b, n_u = ctx.match_pair_device(d_surf, d_pose, n_s, d_fs, d_fp, len(w["fix_surf"]), d_pairs, n_s, d_pf, n_s)
    ctx.window_build(d_surf, d_pose, d_pairs, n_b, w["imu"], w["sample_times"], w["grav"], False, d_fs, d_fp, d_pf, n_u)
    x0 = np.zeros(12 * len(w["sample_times"]))
    ts = []
    for _ in range(5):
        ctx.window_solve(x0)
        ctx.sync()
        t0 = time.perf_counter()
        _, summ, _ = ctx.window_solve(x0)
        ctx.sync()
        ts.append(time.perf_counter() - t0)
    t_solve = sorted(ts)[2]
    out = {"lm_iterations": summ.iterations, "lm_iters_per_s": round(max(1, summ.iterations) / t_solve, 2), "solve_ms": round(t_solve * 1e3, 4)}
    del d_surf, d_pose, d_fs, d_fp, d_pairs, d_pf
    sw = StepWindow(ctx, synth.g2_scan_sequence(10, 3906, m=32, seed=synth.SEED + 21), rank=0, world=1)
    sw.step()
    runs = sorted(sw.step()[0]["solve"] for _ in range(7))
    out["step_solve_ms"] = round(runs[3] * 1e3, 4)
    del sw
    ctx.close()
    out["facade_ms_per_lm_iteration"] = bench.bench_facade_stream(0, False)["ms_per_lm_iteration_median"]
    print(json.dumps(out), flush=True)


def summarize(path):
    rows = [json.loads(l) for l in open(path) if l.startswith("{")]
    figures = []
    for f in ("lm_iters_per_s", "solve_ms", "step_solve_ms", "facade_ms_per_lm_iteration"):
        side = {s: sorted(r[f] for r in rows if r["side"] == s) for s in ("parent", "branch")}
        st = {s: {"min": v[0], "median": (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2, "max": v[-1], "runs": len(v)} for s, v in side.items()}
        spread = st["parent"]["max"] - st["parent"]["min"]
        worse = st["parent"]["median"] - st["branch"]["median"] if f in HIGHER_IS_BETTER else st["branch"]["median"] - st["parent"]["median"]
        figures.append({"figure": f, "better": "higher" if f in HIGHER_IS_BETTER else "lower", "parent": st["parent"], "branch": st["branch"],
                        "parent_spread": round(spread, 4), "branch_median_worse_by": round(worse, 4), "within_bar": worse <= spread})
    print(json.dumps({"what": "the LM loop's decisions moved into csrc/lm_loop.h: parent, branch, parent, ... in fresh processes on one otherwise idle "
                              "MI355X (profiles/dev/ab_lm_loop.sh)",
                      "rule": "per figure, the branch's median is no worse than the parent's median by more than the parent's own max - min",
                      "figures": figures}, indent=1))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(os.path.abspath(os.path.join(ROOT, sys.argv[2])) if len(sys.argv) > 2 else os.path.abspath(ROOT))
    else:
        summarize(sys.argv[2])
