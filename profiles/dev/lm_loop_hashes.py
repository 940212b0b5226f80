"""Same bytes across a change of wc_window_solve's host side: SHA-256 of the returned x and of the wc_solve_summary bytes for
  every scenario of tests/lm_loop_ref.py x {default, lm_dense = 1} x every max_iterations prefix k (0 .. two past the trace's end),
  the window of tests/test_lm_loop_gpu.py::test_sharded_solve_with_rejections on its two thread ranks,
  the bench's C4 window (20 x 50 000 surfels).
python profiles/dev/lm_loop_hashes.py [TREE]   TREE: the root whose wildcat-slam_amd/ is loaded (default: this one; a copy of another
commit with its libraries built, e.g. ab_old).  Run it in fresh processes - the parent's tree twice first, to see that it reproduces
its own hashes - and diff the outputs.  One line per case; the last line is the hash of all lines."""
import hashlib
import os
import sys
import threading

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
TREE = os.path.join(ROOT, sys.argv[1]) if len(sys.argv) > 1 else ROOT
sys.path[:0] = [os.path.join(TREE, "wildcat-slam_amd", "python"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import numpy as np

import lm_loop_ref as ref
import pyoracle
from wildcat_slam_amd import dist as wdist
from wildcat_slam_amd import lib, synth

DEFAULTS = {"lm_dense": 0, "lm_radius0": -1, "lm_dense_radius": 7}
lines = []


def emit(tag, x, s):
    sha = lambda b: hashlib.sha256(b).hexdigest()[:16]
    lines.append("%-44s x %s summary %s  it %d +%d -%d term %d retries %d" % (tag, sha(x.tobytes()), sha(bytes(s)), s.iterations, s.successful_steps,
                                                                          s.unsuccessful_steps, s.termination, int(s.first_step[1])))
    print(lines[-1], flush=True)


def build(c, prob, sharded=False):
    w = prob["w"]
    c.set_params(prob["params"])
    keep = [c.to_device(a) for a in (w["surf"], w["pose"], prob["pairs"], w["fix_surf"], w["fix_pose"], prob["pf"])]
    c.window_build(keep[0], keep[1], keep[2], len(prob["pairs"]), prob["imu"], w["sample_times"], w["grav"], prob["fix_first"], keep[3], keep[4],
                   keep[5], len(prob["pf"]), sharded=sharded)
    return keep


ctx = lib.Context(0)
for name in ref.SCENARIOS:
    prob, trace, want = ref.reference(pyoracle, name)
    keep = build(ctx, prob)
    for form, opts in (("default", {}), ("dense", {"lm_dense": 1})):
        opts = dict(opts)
        if prob["radius0"] != 1e4:
            opts["lm_radius0"] = int(round(np.log10(prob["radius0"])))
        for k in list(range(0, want.iterations + 3)) + [None]:
            ctx.set_params(prob["params"] if k is None else ref.with_max_iterations(prob, k)["params"])
            for o, v in opts.items():
                ctx.set_dev_option(o, v)
            x, s, _ = ctx.window_solve(prob["x0"])
            for o, v in DEFAULTS.items():
                ctx.set_dev_option(o, v)
            emit("%s %s k=%s" % (name, form, "full" if k is None else k), x, s)
    ctx.set_params(prob["params"])
    del keep

# two thread ranks, the two-collective form (late max |g|), next to rejected steps and their dense re-tries
name = next(iter(ref.SCENARIOS))
prob = ref.reference(pyoracle, name)[0]
world = 2
ctxs = [lib.Context(0) for _ in range(world)]
shared = wdist.ThreadComm.shared(world)
res, errors = [None] * world, []


def run(r):
    try:
        c = ctxs[r]
        c.set_comm(wdist.ThreadComm(shared, r, c))
        k = build(c, prob, sharded=True)
        res[r] = c.window_solve(prob["x0"]) + (k,)
    except Exception as e:
        errors.append(e)
        shared["bar"].abort()


th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
for t in th:
    t.start()
for t in th:
    t.join(timeout=120)
assert not errors, errors
for r in range(world):
    emit("%s sharded rank %d of %d" % (name, r, world), res[r][0], res[r][1])
for c in ctxs:
    c.close()

# the bench's C4 window
w = synth.surfel_window(20, 50000, seed=synth.SEED + 7, fixed_patches=50000)
n_s = len(w["surf"])
ctx.close()
ctx = lib.Context(0)  # (the library's own default parameters, as the bench's context has them)
d_surf, d_pose = ctx.to_device(w["surf"]), ctx.to_device(w["pose"])
d_fs, d_fp = ctx.to_device(w["fix_surf"]), ctx.to_device(w["fix_pose"])
d_pairs, d_pf = ctx.alloc(8 * n_s), ctx.alloc(8 * n_s)
n_b, n_u = ctx.match_pair_device(d_surf, d_pose, n_s, d_fs, d_fp, len(w["fix_surf"]), d_pairs, n_s, d_pf, n_s)
ctx.window_build(d_surf, d_pose, d_pairs, n_b, w["imu"], w["sample_times"], w["grav"], False, d_fs, d_fp, d_pf, n_u)
x0 = np.zeros(12 * len(w["sample_times"]))
for rep in range(2):
    x, s, _ = ctx.window_solve(x0)
    emit("C4 20x50000 solve %d" % rep, x, s)
print("all %d cases: %s" % (len(lines), hashlib.sha256("\n".join(lines).encode()).hexdigest()))
ctx.close()
