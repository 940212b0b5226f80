"""Gate clouds for the default extraction path (csrc/extract_fast.inc) - TEST INFRASTRUCTURE.

The default path takes the reference's discrete decisions on its own integer-grid moments and promises that counts and ids stay the
reference's because every decision it cannot trust raises kFlagFxFallback.  The clouds of tests/extract_ref.py keep every gate 1e4 bands
away from its threshold; the clouds built here put ONE gate of ONE node or cluster at a prescribed signed distance from its threshold:

  gate   lam0   the smallest eigenvalue against (double)0.01f: float32 coordinates, so lambda_0 is searched for (tune_lam0: single-ulp
                moves, the fine steps from points close to the mean plane - one ulp of a point at distance d moves lambda_0 by 2 d ulp / n)
         like   min_plane_likeness is a double parameter of the sweep: any patch, the parameter set to its reference likeness -+ delta
         gap    two consecutive stamps of a node cluster_gap + k ticks apart (tick = 2^(e-40) s, the sweep's span < 2^e s), the pair in
                adjacent time bins (phase "adj") or with an empty bin between (phase "skip")
  site   root   the layer-0 root (its children hold <= 20 points each: untested)
         l1     a layer-1 child (the root is no plane by a wide margin)
         l2     a layer-2 child (root and layer-1 parent are no planes by a wide margin).  NOT for lam0: a layer-2 cell is 0.2 m wide, the
                variance of anything inside it is below 0.1^2 = 0.01 along every axis, so lambda_0 < 0.01 - this gate is never near there
         job    a temporal cluster of a plane layer-1 node with two clusters
  class  fall   margin + B <= band: the path MUST hand the sweep to the exact arithmetic (band: extract_ref._band, what fx_pca calls
                "near"; B: the path's own error bound on that quantity, extract_ref.bounds)
         decide margin in [4, 64] x (band + B): it MUST decide itself
         grey   between the two: either is right, the ids must be the reference's
  and, for lam0: "origin" (grey, 1.05 bands out in the voxel at the origin, n = 24: where the band is narrowest), "between" (lambda_0 strictly
  between (double)0.01f and 0.01: the reference says "not a plane"), "slab" (the adversarial cluster, see _slab_case and DESIGN.md 4.3)

Every case is one sweep: the case's voxel, and 64 points in four voxels of 16 (never tested) so that the default path takes the sweep at
all.  case(name) -> dict(points, over (parameter overrides), gate, site, cls, n (the site's point count), layer, margin (signed, measured by
extract_ref.extract in longdouble), band, bound, ref (extract_ref.extract's result), ...).  Nothing here runs on a GPU."""
from fractions import Fraction

import numpy as np

import extract_ref as X
from wildcat_slam_amd import synth

LD = X.LD
VS = float(np.float32(0.8))
THR = float(np.float32(0.01))  # (double)0.01f = 0.00999999977648258...
GAP = 0.05
DT = 1e-4  # between consecutive stamps of a group
T0 = 0.01  # the sweep's first stamp: small stamps (an epoch stamp's ulp, 2.4e-7 s, cannot come near the gap)
REGION = {"root": (0.0, 0.4), "l1": (0.2, 0.2), "l2": (0.3, 0.1)}  # centre (every axis) and half width of the site's cell, voxel-local
LAYER = {"root": 0, "l1": 1, "l2": 2, "job": 1}


class _Params:
    """what extract_ref.extract reads of a wc_params: the defaults the issue names, and a case's overrides"""

    def __init__(self, **over):
        self.voxel_size, self.planer_threshold, self.min_plane_likeness = 0.8, 0.01, 0.1
        self.min_points, self.cluster_min_points, self.cluster_gap, self.max_layer = 20, 20, GAP, 2
        self.view_point = (0.0, 0.0, 0.0)
        for k_, v in over.items():
            setattr(self, k_, v)


def centre(k):
    return (0.5 + np.asarray(k, np.float64)) * VS


def world(k, u):
    return (centre(k) + np.asarray(u, np.float64)).astype(np.float32)


def _ulps(x, m):
    x = np.float32(x)
    to = np.float32(np.inf if m > 0 else -np.inf)
    for _ in range(abs(int(m))):
        x = np.nextafter(x, to)
    return x


def pca_of(p32, c0):
    """one cluster (float32 coordinates, its root voxel's centre) by extract_ref's own arithmetic: centred longdouble moments, Jacobi"""
    d = p32.astype(np.float64).astype(LD) - np.asarray(c0, np.float64).astype(LD)
    n = len(d)
    return X._pca(d, np.zeros(n), np.zeros(n, bool), np.array([0]), np.array([n]), np.asarray(c0, np.float64)[None, :])


def lam0_of(p32, c0):
    """(lambda_0, its eigenvector, likeness) of one cluster"""
    r = pca_of(p32, c0)
    return r["ev"][0, 0], r["V"][0][:, 0].astype(np.float64), r["like"][0]


def tune_lam0(p32, c0, target, tol, movable, max_iter=400, max_m=32):
    """moves coordinates (i, axis) of `movable` by whole ulps until lambda_0 is within tol of target.  Greedy, closed loop: the first-order
    effect of one ulp is 2 (v . (p_i - mean)) v_axis ulp / n; the move whose prediction comes nearest is tried and kept only if the
    MEASURED distance shrinks."""
    p = p32.copy()
    n = len(p)
    lam, v, _ = lam0_of(p, c0)
    for _ in range(max_iter):
        e = float(LD(target) - lam)
        if abs(e) <= tol:
            return p, lam
        pd = p.astype(np.float64)
        d = (pd - pd.mean(axis=0)) @ v
        cands = []
        for i, a in movable:
            s = 2.0 / n * d[i] * v[a] * float(np.spacing(np.abs(p[i, a])))
            if s == 0.0:
                continue
            m = int(max(-max_m, min(max_m, np.rint(e / s))))
            if m:
                cands.append((abs(e - m * s), abs(m), i, a, m))
        cands.sort()
        for _, _, i, a, m in cands[:12]:
            q = p.copy()
            q[i, a] = _ulps(p[i, a], m)
            lam2, v2, _ = lam0_of(q, c0)
            if abs(float(LD(target) - lam2)) < abs(e):
                p, lam, v = q, lam2, v2
                break
        else:
            break
    raise RuntimeError("tune_lam0: lambda_0 - target = %.3g, wanted within %.3g" % (float(lam - LD(target)), tol))


# ---- the default path's moments, restated in exact integers ---------------------------------------------------------------------------
def grid_moments(points, cc):
    """the covariance fx_pca forms: q = rint((p - cc) 2^32) (k_fx_acc's fma: ties to even), every product q_a q_b rounded to nearest-even
    onto the 2^20 grid (units of 2^-44 m^2), exact integer sums, then S / n - m m in float64 in fx_pca's order of operations.
    points (n, 3) float, cc the root voxel's centre -> dict(n, q, s, ss, mean (3), cov (3, 3)): what the kernel holds up to a few fp64 roundings"""
    P = np.asarray(points, np.float64)
    n = len(P)
    cf = [Fraction(float(c)) for c in cc]
    q = [[int(round((Fraction(float(P[i, a])) - cf[a]) * 2**32)) for a in range(3)] for i in range(n)]
    s = [sum(r[a] for r in q) for a in range(3)]
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    ss = [sum(int(round(Fraction(r[a] * r[b], 2**20))) for r in q) for a, b in pairs]
    inn = 1.0 / n
    iq, iqq = 2.0**-32 * inn, 2.0**-44 * inn
    m = [float(s[a]) * iq for a in range(3)]
    C = np.zeros((3, 3))
    for j, (a, b) in enumerate(pairs):
        C[a, b] = C[b, a] = float(ss[j]) * iqq - m[a] * m[b]
    return dict(n=n, q=q, s=s, ss=ss, mean=np.array(m), cov=C)


def grid_lam0(points, cc):
    """the smallest eigenvalue of grid_moments' covariance (longdouble Jacobi: the eigen-solver's own error is not what is predicted)"""
    return float(X.jacobi_eigh(grid_moments(points, cc)["cov"])[0][0, 0])


# ---- pieces of a scene ----------------------------------------------------------------------------------------------------------------
def _flat(rng, site, n, squeeze=1.0, sign_x=0):
    """a thin patch z ~ const filling the site's cell (squeeze < 1: narrower in y - a lower likeness; sign_x: only that half in x)"""
    m, H = REGION[site]
    u = np.empty((n, 3))
    u[:, 0] = m + rng.uniform(-0.85, 0.85, n) * H
    if sign_x:
        u[:, 0] = m + sign_x * rng.uniform(0.1, 0.85, n) * H
    u[:, 1] = m + rng.uniform(-0.85, 0.85, n) * H * squeeze
    u[:, 2] = m + rng.uniform(-0.02, 0.02, n) * H
    return u


def _corners(rng, site, n=20):
    """n points at seven of the eight corners of the site's cell (not + + +, where the next layer's site lies): no plane, by far"""
    m, H = REGION[site]
    sg = [(a, b, c) for a in (-1, 1) for b in (-1, 1) for c in (-1, 1) if (a, b, c) != (1, 1, 1)]
    return np.array([m + H * (0.85 * np.array(sg[i % 7]) + rng.uniform(-0.05, 0.05, 3)) for i in range(n)])


def _lam_cluster(rng, site, n, k):
    """n points (x, y, z) = m + (+-a, +-a, +-h), h ~ 0.1: lambda_0 is the variance of z; ten of them close to the mean plane at distances
    0.1 / 3^j for the fine steps.  world float32 coordinates"""
    m, H = REGION[site]
    a = (0.9 if site == "root" else 0.83) * H  # (a root this wide is one fx_surely_not_plane has to look at twice: 4 det / tr^2 ~ 0.93 lambda_0)
    nt = 10
    sz = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    dz = np.full(n, 0.1)
    dz[n - nt:] = 0.1 / 3.0 ** np.arange(1, nt + 1)
    u = np.empty((n, 3))
    u[:, 0] = m + a * np.where((np.arange(n) // 2) % 2 == 0, 1.0, -1.0) * (1 + rng.uniform(-0.03, 0.03, n))
    u[:, 1] = m + a * np.where((np.arange(n) // 4) % 2 == 0, 1.0, -1.0) * (1 + rng.uniform(-0.03, 0.03, n))
    c0 = centre(k)
    main = np.arange(n) < n - nt
    scale = 1.0
    for _ in range(6):  # the offset of the main points, to first order
        u[:, 2] = m + sz * np.where(main, dz * scale, dz)
        p = world(k, u)
        lam = float(lam0_of(p, c0)[0])
        scale *= np.sqrt(1.0 + (THR - lam) * n / (main.sum() * (0.1 * scale) ** 2))
    return p


def _fillers(rng, k):
    parts = []
    for j, off in enumerate(((3, 0, 0), (0, 3, 0), (3, 3, 0), (0, 0, 3))):
        kk = np.asarray(k) + off
        parts.append((world(kk, rng.uniform(-0.35, 0.35, (16, 3))), T0 + 1e-5 * (16 * j + np.arange(16))))
    return parts


def _stamps(n, t_end):
    return t_end - DT * np.arange(n - 1, -1, -1)


def _assemble(parts):
    xyz = np.concatenate([p for p, _ in parts]).astype(np.float32)
    t = np.concatenate([np.asarray(s, np.float64) for _, s in parts])
    order = np.argsort(t, kind="stable")
    return synth.make_points(xyz[order], t[order])


def tick_of(pts):
    span = float(pts["time"][-1]) - float(pts["time"][0])
    return 2.0 ** (np.frexp(span)[1] - 40)


def time_bin(pts, t):
    """the time bin k_fx_acc puts a stamp in (the hint is the sweep's own range, widened by 4096 ulp)"""
    lo, hi = float(pts["time"][0]), float(pts["time"][-1])
    mag = max(abs(lo), abs(hi))
    t_lo = lo - 4096.0 * (np.nextafter(mag, np.inf) - mag)
    return int((t - t_lo) * (1.0 / (GAP * 0.999)))


# ---- bands and bounds -----------------------------------------------------------------------------------------------------------------
def site_rows(ref, site, n):
    """the rows of extract_ref's stats that are the case's site: (kind, index) with kind "node" / "cluster" """
    S = ref["stats"]
    kinds = ("cluster",) if site == "job" else ("node", "cluster")
    return [(kind, int(i)) for kind in kinds for i in np.flatnonzero((S[kind + "_n"] == n) & (S[kind + "_layer"] == LAYER[site]))]


def lam_bound(ev2, f=0.0):
    """extract_ref.bounds' B_lam for one cluster"""
    return 3 * (2.0**-45 + 2 * 2.0**-33 * VS * f + 16 * 2.0**-53 * (VS / 2) ** 2) + 32 * 2.0**-53 * ev2


def like_band(band, b_lam, tr):
    """the code's dlike = 6 dl / sum + 1e-13, and the path's own likeness error derived the same way from B_lam"""
    return 6.0 * band / tr + 1e-13, 6.0 * b_lam / tr


def classify(margin, band, bound):
    margin = abs(margin)
    if margin + bound <= band:
        return "fall"
    if 4 * (band + bound) <= margin <= 64 * (band + bound):
        return "decide"
    return "grey" if margin < 4 * (band + bound) else "far"


# the signed distance from the threshold every class is built at, in units the class is defined in
def _target(cls, sign, band, bound):
    return sign * {"fall": 0.8 * band, "grey": 2.0 * (band + bound), "decide": 8.0 * (band + bound)}[cls]


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
FAR_K = (25, 0, 0)    # |c| ~ 20 m: the band is wide against the path's own bound - the must-fall-back clusters live here (|c| >= 5 m)
NEAR_K = (0, 0, 0)    # the voxel at the origin, |c| ~ 0.7 m: where the band is narrowest
SIGNS = {"p": 1, "m": -1}


def _names():
    out = []
    for site in ("root", "l1", "job"):
        out += ["lam0-%s-%s-%s" % (site, cls, sg) for cls in ("fall", "grey", "decide") for sg in "pm"]
    out += ["lam0-%s-origin-%s" % (site, sg) for site in ("root", "l1") for sg in "pm"]  # n <= 25 within 2 m of the origin
    out += ["lam0-l1-between", "lam0-root-slab"]
    for site in ("root", "l1", "l2", "job"):
        out += ["like-%s-%s-%s" % (site, cls, sg) for cls in ("fall", "grey", "decide") for sg in "pm"]
    for site in ("root", "l1", "l2"):
        out += ["gap-%s-%s-%s" % (site, ph, k) for ph in ("adj", "skip") for k in ("m16", "m4", "p4", "p16")]
    out += ["gap-bridged-p32"]
    return tuple(out)


CASES = _names()
_CACHE = {}
_SEED = 20240611


def _rng(name):
    return np.random.default_rng([_SEED] + [ord(ch) for ch in name])


def _scene(rng, site, k, cluster_xyz):
    """the case's cluster at its site + what makes every other node of the voxel decide by a wide margin + the fillers"""
    n = len(cluster_xyz)
    t_end = T0 + 1e-3 + DT * n
    parts = _fillers(rng, k) + [(cluster_xyz, _stamps(n, t_end))]
    if site in ("l1", "l2", "job"):  # the root is no plane
        parts.append((world(k, _corners(rng, "root")), _stamps(20, t_end)))
    if site == "l2":  # nor is the layer-1 parent
        parts.append((world(k, _corners(rng, "l1")), _stamps(20, t_end)))
    if site == "job":  # the second temporal cluster of the node: 40 points on its mean plane, 0.1 s later
        parts.append((world(k, _flat(rng, "l1", 40)), _stamps(40, t_end + 0.1 + 40 * DT)))
    return parts


def _xyz(pts):
    return np.stack([pts["x"], pts["y"], pts["z"]], 1)


def _finish(name, gate, site, pts, over, n, k, members, **kw):
    """a PCA-gate case from its sweep: the reference's result, the site's rows, and margin / band / bound / class of the gate it is named for"""
    ref = X.extract(pts, _Params(**over))
    rows = site_rows(ref, site, n)
    assert rows, (name, "the site is not reached")
    S = ref["stats"]
    kind, i = rows[0]
    ev0, like, band = float(S[kind + "_ev0"][i]), float(S[kind + "_like"][i]), float(S[kind + "_band"][i])
    mem = members(pts)
    p = _xyz(pts)[mem]
    r = pca_of(p, centre(k))  # (in longdouble: the rows are rounded to fp64)
    ev = r["ev"][0].astype(np.float64)
    assert len(mem) == n and abs(ev[0] - ev0) <= 1e-17, (name, "the members are not the site's row")
    f = float((np.abs(p) < 2.0**-8).any(axis=1).mean())
    b_lam = lam_bound(ev[2], f)
    c = dict(name=name, gate=gate, site=site, points=pts, over=over, n=n, layer=LAYER[site], ref=ref, rows=rows, ev=ev, f=f,
             centre=p.astype(np.float64).mean(axis=0))
    if gate == "lam0":
        c.update(margin=float(r["ev"][0, 0] - LD(THR)), band=band, bound=b_lam, other_gate=abs(like - _Params(**over).min_plane_likeness))
    else:
        lb, lbound = like_band(band, b_lam, float(ev.sum()))
        c.update(margin=float(r["like"][0] - LD(over["min_plane_likeness"])), band=lb, bound=lbound, other_gate=abs(ev0 - THR))
    c["cls"] = classify(c["margin"], c["band"], c["bound"])
    c.update(kw)
    return c


def _members_of(xyz32):
    """-> function(points) giving the indices of the rows of xyz32 in the assembled cloud, in its order"""
    key = {tuple(r) for r in xyz32.tolist()}

    def find(pts):
        return np.array([i for i, r in enumerate(_xyz(pts).tolist()) if tuple(r) in key], np.int64)

    return find


def _band_at(p32, k):
    c = p32.astype(np.float64).mean(axis=0)
    return float(X._band(np.array([len(p32)]), c[None, :])[0])


def _lam_case(name):
    _, site, cls, *rest = name.split("-")
    rng = _rng(name)
    if cls == "slab":
        return _slab_case(name, rng)
    k = NEAR_K if cls in ("origin", "between") else FAR_K
    n = 24
    region = "l1" if site == "job" else site
    p = _lam_cluster(rng, region, n, k)
    c0 = centre(k)
    band, bound = _band_at(p, k), lam_bound(float(pca_of(p, c0)["ev"][0, 2]))
    if cls == "between":  # strictly between (double)0.01f and 0.01: the reference says "not a plane"
        target = 0.5 * (0.01 - THR)
    elif cls == "origin":  # the grey zone where the band is narrowest, at the band's very edge
        target = SIGNS[rest[0]] * 1.05 * band
    else:
        target = _target(cls, SIGNS[rest[0]], band, bound)
    p, _ = tune_lam0(p, c0, THR + target, 0.02 * abs(target), [(i, a) for i in range(n) for a in range(3)])
    pts = _assemble(_scene(rng, site, k, p))
    return _finish(name, "lam0", site, pts, {}, n, members=_members_of(p), k=k, want=cls)


def _slab_case(name, rng):
    """THE ADVERSARIAL CLUSTER: a root whose normal is the world x axis and whose lower half lies in the slab 0 < x < 2^-9 m, on odd
    multiples of 2^-33 m that the path's 2^-32 m coordinate grid rounds all the same way (ties to even): the path sees the lower half
    2^-33 m nearer the mean than it is, its lambda_0 is 2 (n_low / n) 2^-33 x 0.1 ~ 1e-11 m^2 below the exact one - and the exact one is
    put half that above the threshold.  B_cov's second term (2 2^-33 vs f) is this error; the band has to cover it."""
    k = (0, 3, 2)
    c0 = centre(k)
    n_half, nt = 11, 4
    n = 2 * n_half + nt
    C = int(round(Fraction(float(c0[0])) * 2**32))
    assert Fraction(C, 2**32) == Fraction(float(c0[0]))  # the voxel centre is on the 2^-32 m grid
    # x = (2 j + 1) 2^-33: (x - cc) 2^32 = j + 1/2 - C rounds to the even neighbour; up (+2^-33) where j - C is odd
    j0 = 3 * 2**21  # x ~ 1.5 x 2^-10 m
    js = [j for j in range(j0, j0 + 4 * n_half) if (j - C) % 2 == 1][:n_half]
    x_low = np.array([(2 * j + 1) * 2.0**-33 for j in js])
    u = np.zeros((n, 3))
    a = 0.36
    u[:, 1] = a * np.where((np.arange(n) // 2) % 2 == 0, 1.0, -1.0) * (1 + rng.uniform(-0.03, 0.03, n))
    u[:, 2] = a * np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * (1 + rng.uniform(-0.03, 0.03, n))
    p = world(k, u)
    h = 0.1
    for _ in range(8):  # the distance of the upper half, to first order
        x = np.empty(n)
        x[:n_half] = x_low
        x[n_half:2 * n_half] = float(x_low.mean()) + 2 * h
        x[2 * n_half:] = float(x_low.mean()) + h * (1 + np.array([0.125, -0.03, 0.008, -0.002]))
        p[:, 0] = x.astype(np.float32)
        h *= np.sqrt(THR / float(lam0_of(p, c0)[0]))
    assert np.array_equal(p[:n_half, 0].astype(np.float64), x_low)
    movable = [(i, 0) for i in range(n_half, n)] + [(i, a) for i in range(n) for a in (1, 2)]
    p, _ = tune_lam0(p, c0, THR, 1e-9, movable)  # roughly, then the last steps against the path's own prediction
    err = grid_lam0(p, c0) - float(lam0_of(p, c0)[0])
    assert err < -5e-12, err
    p, lam = tune_lam0(p, c0, THR - 0.5 * err, 0.05 * abs(err), movable)
    pts = _assemble(_scene(rng, "root", k, p))
    c = _finish(name, "lam0", "root", pts, {}, n, members=_members_of(p), k=k, want="adversarial")
    c.update(grid_lam0=grid_lam0(p, c0), cluster=p)
    return c


def _like_case(name):
    _, site, cls, sg = name.split("-")
    rng = _rng(name)
    k = FAR_K
    n = 24
    region = "l1" if site == "job" else site
    p = world(k, _flat(rng, region, n, squeeze=0.6))
    pts = _assemble(_scene(rng, site, k, p))
    find = _members_of(p)
    mem = find(pts)
    r = pca_of(_xyz(pts)[mem], centre(k))
    ev = r["ev"][0].astype(np.float64)
    lb, lbound = like_band(_band_at(p, k), lam_bound(ev[2]), float(ev.sum()))
    over = dict(min_plane_likeness=float(r["like"][0] - LD(_target(cls, SIGNS[sg], lb, lbound))))
    return _finish(name, "like", site, pts, over, n, members=find, k=k, want=cls)


def _gap_case(name):
    _, site, phase, kk = (name.split("-") + ["adj"])[:4] if name.count("-") == 3 else name.replace("bridged", "bridged-adj").split("-")
    rng = _rng(name)
    k = FAR_K
    ticks = (1 if kk[0] == "p" else -1) * int(kk[1:])
    w = GAP * 0.999
    n = 21
    bridged = site == "bridged"
    for tick in (2.0**-42, 2.0**-43, 2.0**-41):  # (the tick follows from the span, the span from the stamps: the first guess holds)
        t1 = T0 + (1.5 if phase == "adj" or bridged else 1.9997) * w
        t2 = t1 + (GAP + ticks * tick)
        parts = _fillers(rng, k)
        if site == "root":  # the pair is the ROOT's alone: the first group in the children x < 0, the second in the children x > 0
            g1, g2 = world(k, _flat(rng, "root", n, sign_x=-1)), world(k, _flat(rng, "root", n, sign_x=1))
            parts += [(g1, _stamps(n, t1)), (g2, t2 + DT * np.arange(n))]
        elif bridged:  # a child that splits (decided on ticks), under a root that does not: a point of another child lies inside the gap
            u1, u2 = _flat(rng, "l1", n), _flat(rng, "l1", n)
            g1, g2 = world(k, u1), world(k, u2)
            parts += [(g1, _stamps(n, t1)), (g2, t2 + DT * np.arange(n)), (world(k, [[-0.2, -0.2, 0.2]]), [t1 + 0.5 * GAP])]
        else:  # the pair is the child's alone: a point of another child (l1) / another layer-2 child (l2) lies inside the gap
            g1, g2 = world(k, _flat(rng, site, n)), world(k, _flat(rng, site, n))
            parts += [(g1, _stamps(n, t1)), (g2, t2 + DT * np.arange(n))]
            for lv in (("root",) if site == "l1" else ("root", "l1")):
                st = _stamps(20, t1)
                if lv == ("root" if site == "l1" else "l1"):
                    st[-1] = t1 + 0.5 * GAP
                parts.append((world(k, _corners(rng, lv)), st))
        pts = _assemble(parts)
        if tick_of(pts) == tick:
            break
    else:
        raise RuntimeError(name + ": no consistent tick")
    ref = X.extract(pts, _Params())
    S = ref["stats"]
    c = dict(name=name, gate="gap", site="l1" if bridged else site, points=pts, over={}, n=2 * n, layer=1 if bridged else LAYER[site], ref=ref, ticks=ticks,
             tick=tick, t1=t1, t2=t2, delta=(t2 - t1) - GAP, bins=(time_bin(pts, t1), time_bin(pts, t2)), phase=phase,
             cls="fall" if abs(ticks) <= 4 else "decide", want="fall" if abs(ticks) <= 4 else "decide", min_gap_dist=S["min_gap_dist"], groups=(g1, g2))
    return c


def case(name):
    if name not in _CACHE:
        _CACHE[name] = {"lam0": _lam_case, "like": _like_case, "gap": _gap_case}[name.split("-")[0]](name)
    return _CACHE[name]
