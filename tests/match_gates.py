"""Gate scenes for the matcher (csrc/match.hip, csrc/match_tree.inc) - TEST INFRASTRUCTURE.

The random scenes of tests/test_match_gpu.py never put a gate's operand within 1e-6 of its threshold.  The scenes built here are rows of
small clusters, 50 m apart along x, and every cluster puts ONE gate of ONE (query, candidate) a prescribed distance from its threshold:

  Q    the query
  N1   its nearest candidate in feature space: one gate at the case's offset, the other two passing by a wide margin
  N2   farther than N1, passes all three by a wide margin
  F    nine surfels farther still, stamped like Q (the time gate rejects them for Q); with them a list of ten stays inside the cluster
  and 64 ordinary surfels far away (the tree gets more than one leaf either way).

A case is LIVE when the restatement (tests/match_ref.py), run on the scene with that one operand on the other side of its threshold,
pairs Q differently: scene(name, same_set, mirror=True) is the same scene with every case's offset mirrored across its threshold, and
because no list of a cluster leaves the cluster (asserted in tests/test_match_ref.py), mirroring all at once is mirroring each alone.

Families.  "A": identity poses, the query's normal along z, clusters on grid-aligned coordinates with z = 0 - qrot, both dot products
and cq - ct are exact, the operand IS the chosen number:
  time   fabs(dt) = time_min + j ulp, j in {0, +-1, +-2, +-4}: stamps near 0 (ulp of time_min; N1 at 0, Q at dt) and, where time_min is
         0.0625, near 1.7e9 s (one ulp of a stamp, 2^-22 s = 2.4e-7 s; N1 at 1.7e9, Q at 1.7e9 + dt, exact)
  angle  the dot product at c* + j ulp, j in -4 .. 4 (c*: the smallest double whose acos is <= ang_max, by bisection; acos is monotone over
         +-2000 ulp around it: c_star asserts it); at cos(ang_max + x 1e-9), x in +-{0.1, 0.5, 2, 10} (straddling the early walk's
         1e-9 rad margin); 1 + 2e-8 from parallel normals of length 1 + 1e-8 and, at 30 deg, -(1 + 2e-8): acos is NaN, NaN passes
  plane  |n . (cq - ct)| at dist_max + j ulp and at dist_max (1 + x 1e-9), same j and x; the clusters' y at 0, 1e3 and 1e5 m in turn
"S": the angle's ulp cases alone (j in -3 .. 3) over a scan of 23 values of ang_max from 0.1 to 179 deg: from 30 deg on one step of
the cosine is one ulp of the angle or less, and an acos that is an ulp off decides otherwise than the host's.
"B": every surfel with a pose of its own (a random rotation, a position ~1e5 m out), general normals; one number of N1 - its stamp, a
component of its body-frame normal, a component of its pose's position - is stepped by ulps over a window, the restated decision is
taken at every step, and the case sits j steps behind the last step of the passing run / in front of the first of the failing run.
Side "band": the early walk accepts on its own arithmetic on the features, off the gates' operands by the features' rounding (a few ulp
of the cosine; of the plane distance, for a center_scale that is no power of two, ~1e-16 of the centre's magnitude); a band case is a
failing step on which the restated early operands (match_ref.early_operands) would pass if cos_acc were cos(ang_max), or if the
1e-9 qmax cs term were missing - where only a margin keeps the walk from being bounded by a candidate the gate rejects.

In same-set scenes the members come as Q, N1, N2 in every other cluster and as N1, N2, Q in the rest (the early walk only accepts a
candidate with an index above the query's).  Nothing here runs on a GPU; scenes are built from seeds."""
import math

import numpy as np

import match_ref as M
from wildcat_slam_amd import records as R

DEG = math.pi / 180.0
STAMP = 1.7e9
STAMP_ULP = 2.0 ** -22
SPACING = 50.0
N_FILL = 9
ULPS = (0, 1, -1, 2, -2, 4, -4)
RELS = (0.1, -0.1, 0.5, -0.5, 2.0, -2.0, 10.0, -10.0)

#        name: (ang_max [deg], dist_max, center_scale, time_min, family)
SCENES = {
    "A0": (5.0, 0.1, 1.0, 0.06, "A"),
    "A1": (0.5, 0.004, 0.5, 0.0625, "A"),
    "A2": (30.0, 0.1, 2.0, 0.06, "A"),
    "A3": (5.0, 0.004, 2.0, 0.0625, "A"),
    "A4": (0.5, 0.1, 1.0, 0.06, "A"),
    "A5": (30.0, 0.004, 0.5, 0.0625, "A"),
    "B0": (5.0, 0.004, 0.3, 0.06, "B"),
    "B1": (30.0, 0.1, 1.0, 0.06, "B"),
    "B2": (0.5, 0.1, 2.0, 0.06, "B"),
}
# family "S": ang_max is a parameter - the dot product at c* + j ulp, j in -3 .. 3, over a scan of angles.  From 30 deg on one ulp of the
# cosine is one ulp of the angle or less: c* - 1 ulp and c* lie within an ulp of ang_max, where an acos that is one ulp off decides otherwise
SCAN_DEG = (0.1, 0.25, 1.0, 2.0, 3.0, 7.5, 10.0, 15.0, 20.0, 25.0, 35.0, 40.0, 45.0, 50.0, 60.0, 70.0, 80.0, 89.0, 90.0, 100.0, 120.0, 150.0, 179.0)
for _deg in SCAN_DEG:
    SCENES["S%05.1f" % _deg] = (_deg, 0.1, 1.0, 0.06, "S")


def ulp(x):
    return float(np.spacing(abs(float(x))))


def _ord(x):
    """the doubles in order: an integer that grows with x (negative numbers mirrored)"""
    i = int(np.array([x], np.float64).view(np.int64)[0])
    return i if i >= 0 else -(i & 0x7FFFFFFFFFFFFFFF)


def _unord(k):
    i = k if k >= 0 else (-k) | (-0x8000000000000000)
    return float(np.array([i], np.int64).view(np.float64)[0])


def step(x, m):
    """x moved m doubles up (m > 0) or down"""
    return _unord(_ord(x) + int(m))


def scene_params(name, k=10):
    ang, dist, cs, tmin, _ = SCENES[name]
    return M.params(knn_k=k, center_scale=cs, angular_scale=ang * DEG, surfel_dist_max=dist, time_diff_min=tmin)


_CSTAR = {}


def c_star(ang):
    """the smallest double c with acos(c) <= ang, and the gaps acos(c* + j ulp) - ang for j in -4 .. 4 in ulp of ang"""
    if ang in _CSTAR:
        return _CSTAR[ang]
    lo, hi = math.cos(ang) - 1e-9, math.cos(ang) + 1e-9  # acos(lo) > ang >= acos(hi)
    assert math.acos(lo) > ang >= math.acos(hi)
    ilo, ihi = _ord(lo), _ord(hi)
    while ihi - ilo > 1:
        mid = (ilo + ihi) // 2
        if math.acos(_unord(mid)) <= ang:
            ihi = mid
        else:
            ilo = mid
    c = _unord(ihi)
    a = [math.acos(step(c, j)) for j in range(-2000, 2001)]
    assert all(x >= y for x, y in zip(a, a[1:])), "acos is not monotone next to c*"
    gaps = {j: (math.acos(step(c, j)) - ang) / ulp(ang) for j in range(-4, 5)}
    _CSTAR[ang] = (c, gaps)
    return _CSTAR[ang]


def _mirror(spec):
    gate, kind, v = spec
    if kind == "ulp" and gate == "time":
        return (gate, kind, (-v[0] - 1, v[1]))
    if kind == "ulp":
        return (gate, kind, 1 - v if gate == "plane" else -v - 1)  # (plane: passes up to 0; time, angle: passes from 0)
    if kind == "rel":
        return (gate, kind, -v)
    if kind == "nan":
        return (gate, "far", v)
    if kind == "far":
        return (gate, "nan", v)
    side, j = v[0], v[1]
    return (gate, kind, ("fail" if side == "pass" else "pass", j) + tuple(v[2:]))


def _specs_a(name):
    ang, dist, cs, tmin, _ = SCENES[name]
    sp = [("time", "ulp", (j, 0.0)) for j in ULPS]
    if tmin == 0.0625:
        sp += [("time", "ulp", (j, STAMP)) for j in ULPS]
    sp += [("angle", "ulp", j) for j in (0, 1, -1, 2, -2, 3, -3, 4, -4)] + [("angle", "rel", x) for x in RELS] + [("angle", "nan", 1)]
    if ang == 30.0:
        sp += [("angle", "nan", -1)]
    sp += [("plane", "ulp", j) for j in ULPS] + [("plane", "rel", x) for x in RELS]
    return sp


def _specs_b(name):
    sp = []
    for gate in ("time", "angle", "plane"):
        sp += [(gate, "nudge", (side, j)) for side in ("pass", "fail") for j in (0, 1, 4)]
    # rejected by the gate, and where only a margin keeps the early walk from accepting (see _cluster_b): many draws, few of them get there
    sp += [("angle", "nudge", ("band", 0, r)) for r in range(24)]
    if SCENES[name][2] == 0.3:
        sp += [("plane", "nudge", ("band", 0, r)) for r in range(48)]
    return sp


def _surfel(c, n, t, pos=(0.0, 0.0, 0.0), quat=(1.0, 0.0, 0.0, 0.0)):
    return dict(c=np.array(c, np.float64), n=np.array(n, np.float64), t=float(t), pos=np.array(pos, np.float64), quat=np.array(quat, np.float64))


def _cluster_a(name, i, spec, rot):
    """family A: -> members [(role, surfel)]; cluster i of its scene"""
    ang, dist, cs, tmin, _ = SCENES[name]
    ang *= DEG
    gate, kind, v = spec
    x = SPACING * i
    y = (0.0, 1e3, 1e5)[(i + rot) % 3]
    base = (0.0, STAMP)[i % 2]
    tq, t1, t2 = base + 1.0, base, base + 0.25
    nq, n1 = (0.0, 0.0, 1.0), (0.0, 0.0, 1.0)
    c1 = [x, y + 0.125 * cs, 0.0]
    o2, fill0, fstep = 1.5, 3.0, 0.75  # N2's and the fillers' offsets along y, in feature units
    if gate == "time":
        j, base = v
        dt = tmin + j * (ulp(tmin) if base == 0.0 else STAMP_ULP)
        tq, t1, t2 = base + dt, base, base - 0.5
        assert tq - t1 == dt
    elif gate == "angle":
        if kind in ("nan", "far"):
            ln = 1.0 + 1e-8
            nq = (0.0, 0.0, ln)
            if kind == "nan":
                n1 = (0.0, 0.0, v * ln)
            else:  # the mirror of a NaN case: rejected by a wide margin
                cth, sth = math.cos(2.0 * ang), math.sin(2.0 * ang)
                n1 = (v * sth, 0.0, v * cth)
            if v < 0:
                o2, fill0, fstep = 5.0, 6.0, 0.5
        else:
            c = step(c_star(ang)[0], v) if kind == "ulp" else math.cos(ang + v * 1e-9)
            n1 = (math.sqrt(1.0 - c * c), 0.0, c)
    else:
        h = step(dist, v) if kind == "ulp" else dist * (1.0 + v * 1e-9)
        c1[2] = h if i % 4 < 2 else -h
    mem = [("Q", _surfel((x, y, 0.0), nq, tq)), ("N1", _surfel(c1, n1, t1)), ("N2", _surfel((x, y + o2 * cs, 0.0), (0.0, 0.0, 1.0), t2))]
    for f in range(N_FILL):
        off = (fill0 + fstep * (f // 2)) * (1.0 if f % 2 == 0 else -1.0)
        mem.append(("F", _surfel((x, y + off * cs, 0.0), (0.0, 0.0, 1.0), tq)))
    return mem


def _rand_quat(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def _qmat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _posed(rng, cw, nw, t):
    """a surfel whose world centre and normal come out near (cw, nw) through a pose of its own"""
    q = _rand_quat(rng)
    Rm = _qmat(q)
    pos = np.asarray(cw) - Rm @ (rng.uniform(-5.0, 5.0, size=3))
    return _surfel(Rm.T @ (np.asarray(cw) - pos), Rm.T @ np.asarray(nw), t, pos, q)


def _records(members):
    n = len(members)
    s, p = np.zeros(n, R.SURFEL), np.zeros(n, R.POSE)
    for i, m in enumerate(members):
        s["center"][i], s["normal"][i], s["t"][i], p["pos"][i], p["quat"][i] = m["c"], m["n"], m["t"], m["pos"], m["quat"]
    s["resolution"], s["sigma"] = 0.4, 0.005
    return s, p


def _cluster_b(name, i, spec, rng):
    """family B: general poses and normals; one number of N1 stepped to the prescribed place"""
    ang, dist, cs, tmin, _ = SCENES[name]
    ang *= DEG
    gate, _, v = spec
    side, j = v[0], v[1]
    big = 1e5 if name != "B1" else 1e3
    P0 = np.array([0.61 * big + SPACING * i, big, -0.37 * big]) + rng.uniform(-1.0, 1.0, size=3)
    n = rng.normal(size=3)
    n /= np.linalg.norm(n)
    e = np.cross(n, [1.0, 0.0, 0.0])  # in the query's plane and across the row of clusters
    e /= np.linalg.norm(e)
    e2 = np.cross(n, e)
    base = (0.37, STAMP + 0.37)[i % 2]
    tq, t1, t2 = base + 1.0, base, base + 0.25
    n1w, c1w = n, P0 + 0.125 * cs * e
    if gate == "time":
        t1 = tq - tmin
    elif gate == "angle":
        n1w = math.cos(ang) * n + math.sin(ang) * e2  # (tilted about e: e stays in both planes)
    else:
        c1w = c1w + dist * n * (1.0 if i % 4 < 2 else -1.0)
    q_s = _posed(rng, P0, n, tq)
    n1_s = _posed(rng, c1w, n1w, t1)
    # the decision at every step of the window
    W = 512
    ms = np.arange(-W, W + 1)
    var = [dict(n1_s, c=n1_s["c"].copy(), n=n1_s["n"].copy(), pos=n1_s["pos"].copy()) for _ in ms]
    if gate == "time":
        for m, s in zip(ms, var):
            s["t"] = step(n1_s["t"], m)
    elif gate == "angle":
        a = int(np.argmax(np.abs(n1_s["n"])))
        for m, s in zip(ms, var):
            s["n"][a] = step(n1_s["n"][a], m)
    else:
        qw = M.world(*_records([q_s]))[1][0]
        # (along the axis where the query's normal is smallest but not negligible: the finest steps of the operand the world centre's ulp allows)
        a = int(np.argmin(np.where(np.abs(qw) >= 0.05, np.abs(qw), 2.0)))
        for m, s in zip(ms, var):
            s["pos"][a] = step(n1_s["pos"][a], m)
    vs, vp = _records(var)
    qs, qp = _records([q_s])
    cw, nw = M.world(vs, vp)
    qc, qn = M.world(qs, qp)
    if gate == "time":
        dec = ~(np.abs(vs["t"] - qs["t"][0]) < tmin)
    elif gate == "angle":
        dec = (qn[0, 0] * nw[:, 0] + qn[0, 1] * nw[:, 1] + qn[0, 2] * nw[:, 2]) >= c_star(ang)[0]
    else:
        d = qc[0] - cw
        dec = ~(np.abs(qn[0, 0] * d[:, 0] + qn[0, 1] * d[:, 1] + qn[0, 2] * d[:, 2]) > dist)
    if not dec[0]:
        dec, var = dec[::-1], var[::-1]
    assert dec[0] and not dec[-1], (name, spec, "the window does not hold the threshold")
    last_pass = int(np.argmin(dec)) - 1  # the end of the leading run of passes
    first_fail = len(dec) - int(np.argmax(dec[::-1]))  # the start of the trailing run of failures
    pick = last_pass - j if side == "pass" else first_fail + j
    if side == "band":
        # a failing step on which the early walk's own operands (match_ref.early_operands) would pass without their margins: the cosine
        # against cos(ang_max), the plane distance against plane_acc without the 1e-9 qmax cs term.  Where the window holds none (most
        # draws: the features' rounding has to outweigh the operand's distance from the threshold) the case stays the first failing step.
        P = scene_params(name)
        ws, wp = _records(var)
        e_cos, e_pl, qmax = M.early_operands(M.features(qs, qp, P)[0], M.features(ws, wp, P), P)
        cos_acc, plane_acc = M.early_margins(P)
        if gate == "angle":
            inside = ~dec & (e_cos >= math.cos(ang)) & (e_pl <= dist - 1e-9 * qmax * cs)
        else:
            inside = ~dec & (e_cos >= cos_acc) & (e_pl <= plane_acc)
        if inside.any():
            pick = int(np.argmax(inside))
    n1_s = var[pick]
    mem = [("Q", q_s), ("N1", n1_s), ("N2", _posed(rng, P0 + 1.5 * cs * e, n, t2))]
    for f in range(N_FILL):
        off = (3.0 + 0.75 * (f // 2)) * (1.0 if f % 2 == 0 else -1.0)
        mem.append(("F", _posed(rng, P0 + off * cs * e, n, tq)))
    return mem


def _padding(rng, n, t_lo, t_hi):
    mem = []
    for _ in range(n):
        nn = rng.normal(size=3)
        mem.append(_surfel(np.array([-5000.0, 0.0, 0.0]) + rng.uniform(-20.0, 20.0, size=3), nn / np.linalg.norm(nn), rng.uniform(t_lo, t_hi)))
    return mem


_CACHE = {}


def scene(name, same_set, mirror=False):
    """-> dict(name, same_set, q_surf, q_pose, t_surf, t_pose, cases [dict(id, gate, kind, value, q, n1, n2, members (target indices of the
    cluster), first (Q in front of N1 and N2))]); in a same-set scene q_* are t_*"""
    key = (name, bool(same_set), bool(mirror))
    if key in _CACHE:
        return _CACHE[key]
    fam = SCENES[name][4]
    specs = _specs_a(name) if fam == "A" else _specs_b(name) if fam == "B" else [("angle", "ulp", j) for j in (0, 1, -1, 2, -2, 3, -3)]
    rng = np.random.default_rng(1000 + sorted(SCENES).index(name))  # (the same draws with and without the mirror)
    targets, queries, cases = [], [], []
    for i, spec in enumerate(specs):
        sp = _mirror(spec) if mirror else spec
        mem = _cluster_a(name, i, sp, sorted(SCENES).index(name)) if fam != "B" else _cluster_b(name, i, sp, np.random.default_rng([7, sorted(SCENES).index(name), i]))
        first = i % 2 == 0
        if same_set and not first:
            mem = [mem[1], mem[2], mem[0]] + mem[3:]
        case = dict(id="%s/%d %s %s %s" % (name, i, spec[0], spec[1], spec[2]), gate=spec[0], kind=spec[1], value=spec[2], first=first, members=[])
        for role, s in mem:
            if role == "Q" and not same_set:
                case["q"] = len(queries)
                queries.append(s)
                continue
            if role == "Q":
                case["q"] = len(targets)
            elif role == "N1":
                case["n1"] = len(targets)
            elif role == "N2":
                case["n2"] = len(targets)
            case["members"].append(len(targets))
            targets.append(s)
        cases.append(case)
    if same_set:
        targets += _padding(rng, 64, 0.0, 5.0)
    else:
        targets += _padding(rng, 64, 0.0, 5.0)
        queries += _padding(rng, 16, 10.0, 15.0)
    t_surf, t_pose = _records(targets)
    q_surf, q_pose = (t_surf, t_pose) if same_set else _records(queries)
    sc = dict(name=name, same_set=bool(same_set), q_surf=q_surf, q_pose=q_pose, t_surf=t_surf, t_pose=t_pose, cases=cases)
    _CACHE[key] = sc
    return sc


GATE_COL = {"time": 0, "angle": 1, "plane": 2}


def measure(sc, ref, P):
    """per case, from a match_ref.match result of the scene at k >= 3: where N1 stands in Q's list, which side the restatement puts the
    case's gate on, and how far its operand is from the threshold (ulp of the threshold; the angle also in ulp of ang_max)"""
    out = []
    cst = c_star(P.angular_scale)[0]
    for c in sc["cases"]:
        q, row = c["q"], list(ref["idx"][c["q"]])
        j1 = row.index(c["n1"])
        g = GATE_COL[c["gate"]]
        m = dict(id=c["id"], pos=j1, passed=bool(ref["passed"][q, j1, g]), others=bool(np.delete(ref["passed"][q, j1], g).all()))
        if c["gate"] == "time":
            m["ulp"] = (ref["dt"][q, j1] - P.time_diff_min) / ulp(P.time_diff_min)
        elif c["gate"] == "angle":
            m["ulp"] = float(_ord(ref["dot"][q, j1]) - _ord(cst))  # (in doubles: c* may sit on a power of two)
            m["ulp_ang"] = (ref["ang"][q, j1] - P.angular_scale) / ulp(P.angular_scale)
        else:
            m["ulp"] = (ref["plane"][q, j1] - P.surfel_dist_max) / ulp(P.surfel_dist_max)
        j2 = row.index(c["n2"])
        m["n2_pos"], m["n2_passes"] = j2, bool(ref["passed"][q, j2].all())
        out.append(m)
    return out


def pairs_of(pairs, sc, case):
    """the pairs of a result that Q of the case is part of, as a sorted list of tuples"""
    q = case["q"]
    col = "second" if not sc["same_set"] else None
    if col:
        return sorted((int(a), int(b)) for a, b in zip(pairs["first"], pairs["second"]) if b == q)
    return sorted((int(a), int(b)) for a, b in zip(pairs["first"], pairs["second"]) if a == q or b == q)


def describe(sc, case, got, ref):
    """one line of a failure message: the gate, the offset, and which of Q's candidates each side took"""
    def who(ps):
        names = []
        for a, b in ps:
            o = a if (sc["same_set"] and b == case["q"]) or not sc["same_set"] else b
            names.append("N1" if o == case["n1"] else "N2" if o == case["n2"] else "#%d" % o)
        return "+".join(names) or "nobody"

    return "%s: GPU pairs Q with %s, the reference with %s" % (case["id"], who(pairs_of(got, sc, case)), who(pairs_of(ref, sc, case)))


# ---- tie scenes: exactly equal feature distances, cut by the gates ---------------------------------------------------------------------
_AXES = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, -1.0]])


def _lattice(rng, n, cells, t0):
    """n surfels on a 0.25 m lattice of cells^3 sites, normals along the axes, stamps t0 or t0 + 0.5 by the parity of the index"""
    s, p = np.zeros(n, R.SURFEL), np.zeros(n, R.POSE)
    s["center"] = rng.integers(0, cells, size=(n, 3)) * 0.25
    s["normal"] = _AXES[rng.integers(0, 6, size=n)]
    s["t"] = t0 + 0.5 * (np.arange(n) % 2)
    s["resolution"], s["sigma"] = 0.4, 0.005
    p["quat"][:, 0] = 1.0
    return s, p


def tie_scene(kind, same_set):
    """kind "block": 3 000 surfels, 1 500 of them with ONE centre and normal (indices 700 .. 2 199: one bucket of the tree, all their
    distances tie and the lists are decided by the index alone), the others on a 0.25 m lattice of 12^3 sites with normals along the
    axes (many sites hold several surfels, and neighbours at +-x, +-y, +-z tie); kind "few": seven targets, three of them coincident,
    two pairs symmetric about them - fewer than k for k = 10 and 16.  The stamps differ by 0 or 0.5 s by the parity of the index and
    time_min lies between: the time gate fails about half of every tied group.  Two sets: the queries lie on the same lattice, 10.5 s
    on, and time_min is 10.25 s (passes the even targets).  -> dict like scene(), with P (match_ref.params at k = 16)"""
    rng = np.random.default_rng(42 if kind == "block" else 43)
    if kind == "block":
        t_surf, t_pose = _lattice(rng, 3000, 12, 0.0)
        t_surf["center"][700:2200] = t_surf["center"][700]
        t_surf["normal"][700:2200] = t_surf["normal"][700]
        nq = 900
    else:
        t_surf, t_pose = _lattice(rng, 7, 2, 0.0)
        t_surf["normal"][:] = _AXES[2]
        t_surf["center"][:] = np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [1.25, 1.0, 0.0], [0.75, 1.0, 0.0], [1.0, 1.25, 0.0], [1.0, 0.75, 0.0]])
        nq = 5
    if same_set:
        q_surf, q_pose, tmin = t_surf, t_pose, 0.25
    else:
        q_surf, q_pose = _lattice(rng, nq, 12 if kind == "block" else 2, 10.5)
        q_surf["t"] = 10.5
        if kind == "block":
            q_surf["center"][100:400] = t_surf["center"][700]
            q_surf["normal"][100:400] = t_surf["normal"][700]
        else:
            q_surf["normal"][:] = _AXES[2]
            q_surf["center"][:] = np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [1.125, 1.0, 0.0], [1.0, 1.125, 0.0], [0.0, 0.0, 0.0]])
        tmin = 10.25
    return dict(name="ties-" + kind, same_set=bool(same_set), q_surf=q_surf, q_pose=q_pose, t_surf=t_surf, t_pose=t_pose, cases=[],
                P=M.params(knn_k=16, time_diff_min=tmin))
