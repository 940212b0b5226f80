"""High-precision reference of the whole surfel extraction (BuildSurfels, surfel_extraction.cc:316-337) - TEST INFRASTRUCTURE.

Written from SURVEY.md Appendix A and oracle/extract.cc in plain numpy.  The DECISIONS are the reference's (root voxels by the true fp64
division, float quarter lengths, strict comparisons, n > min_points, the root split whether or not it is a plane, temporal clusters by
the fp64 difference of consecutive stamps of a node, n >= cluster_min_points, both gates, orientation towards the view point, ids in the
oracle's encoding); the ARITHMETIC behind them is not:
  * moments are centred, two-pass (with the correction term) about the root voxel's centre in numpy.longdouble (64-bit mantissa);
  * the stamp mean is formed about the cluster's first stamp;
  * the eigen-decomposition is a cyclic Jacobi iteration in longdouble, run until the off-diagonal entries are below 1e-19 of the trace.
Nothing here knows the integer grids of csrc/extract_fast.inc: what the default path returns is measured against this, field by field
(tests/test_extract_precision_gpu.py), and this module is itself held against exact rational moments (tests/test_extract_ref.py).

extract(points, params) -> dict, one row per surfel in the oracle's output order (stamp, then id):
  ids (SURFEL_ID), surfels (SURFEL, rounded to fp64: for helpers.check_surfels), n, layer, f (share of the cluster's points with a
  coordinate below 2^-8 m in magnitude), and in longdouble: t, center, cov (3 x 3), ev (ascending), evecs (columns, as the iteration left
  them), normal (evecs[:, 0], oriented), sigma2 (= ev[0], NOT
  its root: a NaN is never this reference's answer), orient (normal . (centre - view) before orienting), members (point indices);
  stats: root_voxels, nodes_tested / nodes_plane per layer, clusters_total / clusters_rejected, surfels, min_gate_margin (as oracle/extract.cc),
  node_* and cluster_* arrays (n, centre, margin = distance of the nearer gate from its threshold, like, ev0, band = the width
  16 sqrt(n) (|c|^2 + 1) 2^-53 + 1e-14 + 3 B_cov(f = 1) inside which the default path hands the sweep to the exact arithmetic), min_gap_dist (the
  smallest | (t_i - t_{i-1}) - cluster_gap | over consecutive stamps of every tested node)."""
from fractions import Fraction

import numpy as np

from wildcat_slam_amd import records as R

LD = np.longdouble
if np.finfo(LD).nmant < 63:
    raise RuntimeError("numpy.longdouble is no wider than double here (%d mantissa bits): extract_ref would compare the default "
                       "path with arithmetic of its own precision" % np.finfo(LD).nmant)


def jacobi_eigh(A, tol=1e-19, max_sweeps=60):
    """cyclic Jacobi iteration on a batch of symmetric 3 x 3 matrices (M, 3, 3) in longdouble -> (ev (M, 3) ascending, V (M, 3, 3) with
    the eigenvectors in the columns).  Stops when every off-diagonal entry is below tol x the sum of the diagonal's magnitudes."""
    A = np.array(A, LD).reshape(-1, 3, 3).copy()
    A = (A + A.transpose(0, 2, 1)) / LD(2)
    M = len(A)
    V = np.zeros((M, 3, 3), LD)
    V[:, [0, 1, 2], [0, 1, 2]] = 1
    one = LD(1)
    with np.errstate(all="ignore"):
        for _ in range(max_sweeps):
            off = np.maximum(np.maximum(np.abs(A[:, 0, 1]), np.abs(A[:, 0, 2])), np.abs(A[:, 1, 2]))
            tr = np.abs(A[:, 0, 0]) + np.abs(A[:, 1, 1]) + np.abs(A[:, 2, 2])
            if np.all(off <= LD(tol) * tr):
                break
            for p, q in ((0, 1), (0, 2), (1, 2)):
                apq = A[:, p, q]
                nz = apq != 0
                theta = (A[:, q, q] - A[:, p, p]) / (LD(2) * apq)
                tt = np.where(theta >= 0, one, -one) / (np.abs(theta) + np.sqrt(theta * theta + one))
                tt = np.where(np.isfinite(tt), tt, LD(0))
                c = one / np.sqrt(tt * tt + one)
                s = tt * c
                c, s = np.where(nz, c, one), np.where(nz, s, LD(0))
                J = np.zeros((M, 3, 3), LD)
                J[:, [0, 1, 2], [0, 1, 2]] = 1
                J[:, p, p], J[:, q, q], J[:, p, q], J[:, q, p] = c, c, s, -s
                A = np.einsum("mji,mjk,mkl->mil", J, A, J)
                A[:, p, q] = np.where(nz, LD(0), A[:, p, q])
                A[:, q, p] = A[:, p, q]
                A = (A + A.transpose(0, 2, 1)) / LD(2)
                V = np.einsum("mij,mjk->mik", V, J)
        else:
            raise RuntimeError("jacobi_eigh did not converge")
    d = A[:, [0, 1, 2], [0, 1, 2]]
    order = np.argsort(d, axis=1, kind="stable")
    ev = np.take_along_axis(d, order, 1)
    V = np.take_along_axis(V, order[:, None, :], 2)
    V = V / np.sqrt((V * V).sum(axis=1, keepdims=True))
    return ev, V


def ld_to_fraction(x):
    """exact value of a longdouble as a Fraction (two doubles: the 64-bit mantissa splits into 53 + 11 bits)"""
    x = LD(x)
    hi = float(x)
    lo = float(x - LD(hi))
    assert LD(hi) + LD(lo) == x
    return Fraction(hi) + Fraction(lo)


def _segments(lab_sorted):
    starts = np.flatnonzero(np.concatenate([[True], lab_sorted[1:] != lab_sorted[:-1]]))
    counts = np.diff(np.concatenate([starts, [len(lab_sorted)]]))
    return starts, counts


def _pca(d, t, f_small, starts, counts, root_c):
    """centred two-pass moments of the contiguous groups (starts, counts) of d = p - root centre (longdouble), and their eigen-decomposition"""
    n = counts.astype(LD)
    md = np.add.reduceat(d, starts, axis=0) / n[:, None]
    e = d - np.repeat(md, counts, axis=0)
    me = np.add.reduceat(e, starts, axis=0) / n[:, None]
    S = np.add.reduceat(e[:, :, None] * e[:, None, :], starts, axis=0) / n[:, None, None] - me[:, :, None] * me[:, None, :]
    c = root_c.astype(LD) + (md + me)
    t0 = t[starts]
    tm = t0.astype(LD) + np.add.reduceat(t.astype(LD) - np.repeat(t0, counts).astype(LD), starts) / n
    ev, V = jacobi_eigh(S)
    with np.errstate(all="ignore"):
        like = LD(2) * (ev[:, 1] - ev[:, 0]) / ((ev[:, 0] + ev[:, 1]) + ev[:, 2])
    f = np.add.reduceat(f_small.astype(np.float64), starts) / counts
    return dict(n=counts.copy(), center=c, cov=S, ev=ev, V=V, like=like, t=tm, f=f)


def _band(n, c, vs=0.8):
    """the width of fx_pca's "near a gate" band (csrc/extract_fast.inc), as DESIGN.md 4.3 states it: 16 x the reference's rounding noise, and
    the default path's own error on lambda_0 - 3 B_cov of bounds() below, with f = 1 (a constant of the sweep)"""
    c = np.asarray(c, np.float64)
    vs = float(np.float32(vs))
    grid = 3.0 * (2.0**-45 + 2 * 2.0**-33 * vs + 16 * 2.0**-53 * (vs / 2) ** 2)
    return 16.0 * np.sqrt(np.asarray(n, np.float64)) * ((c * c).sum(axis=1) + 1.0) * 2.0**-53 + 1e-14 + grid


def extract(points, params):
    vs32 = np.float32(params.voxel_size)
    vs = np.float64(vs32)
    thr = LD(np.float64(np.float32(params.planer_threshold)))
    min_like = LD(np.float64(params.min_plane_likeness))
    minp, cmin, gap, max_layer = int(params.min_points), int(params.cluster_min_points), np.float64(params.cluster_gap), int(params.max_layer)
    view = np.array([params.view_point[i] for i in range(3)], np.float64)
    fin = np.isfinite(np.stack([points["x"], points["y"], points["z"]], 1)).all(axis=1)
    if not fin.all():  # a point with a non-finite coordinate contributes to nothing (the reference bins it with its own kind: no gate passes)
        res = extract(points[fin], params)
        idx = np.flatnonzero(fin)
        res["members"] = [idx[m_] for m_ in res["members"]]
        return res
    N = len(points)
    p = np.stack([points["x"], points["y"], points["z"]], 1).astype(np.float64)
    t = np.ascontiguousarray(points["time"], np.float64)
    k = np.floor(p / vs).astype(np.int64)
    uniq, g0 = np.unique(k, axis=0, return_inverse=True)
    g0 = g0.reshape(-1)
    c0 = (0.5 + uniq) * vs
    quarter = [vs32 / np.float32(4)]
    quarter += [quarter[0] / np.float32(2), quarter[0] / np.float32(4)]
    b1 = p > c0[g0]
    o1 = 4 * b1[:, 0] + 2 * b1[:, 1] + 1 * b1[:, 2]
    c1 = c0[g0] + ((2 * b1 - 1).astype(np.float32) * quarter[0]).astype(np.float64)
    b2 = p > c1
    o2 = 4 * b2[:, 0] + 2 * b2[:, 1] + 1 * b2[:, 2]
    labs = [g0.astype(np.int64), g0 * 8 + o1, (g0 * 8 + o1) * 8 + o2]
    codes = [np.zeros(N, np.int64), 1 | (o1 << 2), 2 | (o1 << 2) | (o2 << 5)]
    d = p.astype(LD) - c0[g0].astype(LD)
    f_small = (np.abs(p) < 2.0**-8).any(axis=1)

    stats = dict(root_voxels=len(uniq), nodes_tested=[0, 0, 0], nodes_plane=[0, 0, 0], clusters_total=0, clusters_rejected=0)
    node_rows, cluster_rows, out, all_sizes = [], [], [], []
    min_gap_dist = np.inf
    mask = np.ones(N, bool)
    for layer in range(min(max_layer, 2) + 1):
        lab = labs[layer]
        cnt = np.bincount(lab, weights=mask, minlength=int(lab.max()) + 1 if N else 1)
        tested_pt = mask & (cnt[lab] > minp)
        idx = np.flatnonzero(tested_pt)
        plane_pt = np.zeros(N, bool)
        if len(idx):
            order = idx[np.argsort(lab[idx], kind="stable")]  # stable: every node keeps the input order of its points
            starts, counts = _segments(lab[order])
            r = _pca(d[order], t[order], f_small[order], starts, counts, c0[g0[order[starts]]])
            is_plane = (r["ev"][:, 0] < thr) & (r["like"] > min_like)
            margin = np.minimum(np.abs(r["ev"][:, 0] - thr), np.abs(r["like"] - min_like)).astype(np.float64)
            stats["nodes_tested"][layer] = len(starts)
            stats["nodes_plane"][layer] = int(is_plane.sum())
            node_rows.append(dict(n=counts, center=r["center"].astype(np.float64), margin=margin, like=r["like"].astype(np.float64),
                                  ev0=r["ev"][:, 0].astype(np.float64), layer=np.full(len(starts), layer)))
            first = np.zeros(len(order), bool)
            first[starts] = True
            dt = np.concatenate([[0.0], t[order][1:] - t[order][:-1]])
            if (~first).any():
                min_gap_dist = min(min_gap_dist, float(np.abs(dt[~first] - gap).min()))
            plane_sorted = np.repeat(is_plane, counts)
            plane_pt[order[plane_sorted]] = True
            # temporal clusters of the plane nodes (ClusterSurfels)
            po, pfirst, pdt = order[plane_sorted], first[plane_sorted], dt[plane_sorted]
            if len(po):
                new = pfirst | (pdt > gap)
                gid = np.cumsum(new) - 1
                node_first_gid = np.maximum.accumulate(np.where(pfirst, gid, 0))
                ci = gid - node_first_gid
                ccount = np.bincount(gid)
                stats["clusters_total"] += len(ccount)
                all_sizes.append(ccount)
                keep = ccount[gid] >= cmin
                ko, kci = po[keep], ci[keep]
                if len(ko):
                    cs, cc = _segments(gid[keep])
                    q = _pca(d[ko], t[ko], f_small[ko], cs, cc, c0[g0[ko[cs]]])
                    cm = np.minimum(np.abs(q["ev"][:, 0] - thr), np.abs(q["like"] - min_like)).astype(np.float64)
                    rej = (q["ev"][:, 0] > thr) | (q["like"] < min_like)
                    stats["clusters_rejected"] += int(rej.sum())
                    cluster_rows.append(dict(n=cc, center=q["center"].astype(np.float64), margin=cm, like=q["like"].astype(np.float64),
                                             ev0=q["ev"][:, 0].astype(np.float64), layer=np.full(len(cs), layer)))
                    for j in np.flatnonzero(~rej):
                        pt0 = ko[cs[j]]
                        out.append(dict(key=uniq[g0[pt0]], node=int(codes[layer][pt0]) | (int(kci[cs[j]]) << 8), layer=layer, n=int(cc[j]), f=float(q["f"][j]),
                                        t=q["t"][j], center=q["center"][j], cov=q["cov"][j], ev=q["ev"][j], normal=q["V"][j][:, 0], evecs=q["V"][j],
                                        members=ko[cs[j]:cs[j] + cc[j]]))
        else:
            is_plane = np.zeros(0, bool)
        mask = tested_pt if layer == 0 else (tested_pt & ~plane_pt)  # the root is split whether or not it is a plane (Q4)

    def cat(rows, key):
        return np.concatenate([r[key] for r in rows]) if rows else np.zeros(0)

    for name, rows in (("node", node_rows), ("cluster", cluster_rows)):
        for key in ("n", "center", "margin", "like", "ev0", "layer"):
            stats[name + "_" + key] = cat(rows, key) if key != "center" else (np.concatenate([r[key] for r in rows]) if rows else np.zeros((0, 3)))
        stats[name + "_band"] = _band(stats[name + "_n"], stats[name + "_center"], vs)
    margins = np.concatenate([stats["node_margin"], stats["cluster_margin"]])
    stats["min_gate_margin"] = float(margins.min()) if len(margins) else 1e300
    stats["min_gap_dist"] = min_gap_dist
    stats["cluster_sizes_all"] = np.concatenate(all_sizes) if all_sizes else np.zeros(0, np.int64)  # (the clusters below cluster_min_points too)
    stats["surfels"] = len(out)

    M = len(out)
    ids = np.zeros(M, R.SURFEL_ID)
    s = np.zeros(M, R.SURFEL)
    res = dict(n=np.zeros(M, np.int64), layer=np.zeros(M, np.int64), f=np.zeros(M), t=np.zeros(M, LD), center=np.zeros((M, 3), LD), cov=np.zeros((M, 3, 3), LD),
               ev=np.zeros((M, 3), LD), normal=np.zeros((M, 3), LD), evecs=np.zeros((M, 3, 3), LD), orient=np.zeros(M, LD))
    for i, o in enumerate(out):
        ids[i] = (o["key"][0], o["key"][1], o["key"][2], o["node"])
        for key in ("n", "layer", "f", "t", "center", "cov", "ev", "normal", "evecs"):
            res[key][i] = o[key]
    res["orient"] = (res["normal"] * (res["center"] - view.astype(LD))).sum(axis=1)
    res["normal"] = np.where((res["orient"] < 0)[:, None], -res["normal"], res["normal"])
    res["sigma2"] = res["ev"][:, 0].copy()
    s["t"], s["center"], s["cov"], s["normal"] = res["t"].astype(np.float64), res["center"].astype(np.float64), res["cov"].reshape(M, 9).astype(np.float64), res["normal"].astype(np.float64)
    s["resolution"] = np.array([np.float64(quarter[l] * np.float32(4)) for l in res["layer"]]) if M else np.zeros(0)
    s["sigma"] = np.sqrt(np.maximum(res["sigma2"], LD(0))).astype(np.float64)
    order = np.lexsort((ids["node"], ids["kz"], ids["ky"], ids["kx"], s["t"]))  # by stamp, ties by id
    members = [out[i]["members"] for i in order]
    res = {k_: v[order] for k_, v in res.items()}
    res.update(ids=ids[order], surfels=s[order], members=members, stats=stats)
    assert not any(np.isnan(np.asarray(res[k_], np.float64)).any() for k_ in ("t", "center", "cov", "ev", "normal", "sigma2"))
    return res


# ---- the clouds of the precision tests ------------------------------------------------------------------------------------------------
# name -> (points, parameter overrides).  Tens of thousands of points at most; what each one is there for is said next to it, and
# tests/test_extract_ref.py asserts that it does reach it (layers, cluster counts, gate margins, stamp gaps).
CLOUDS = ("lattice095", "q4", "revisits3", "room", "epoch", "far", "straddle", "dense", "edges", "planar")
FAR_SHIFT = 526 * 0.95  # ~500 m: a whole number of 0.95 m root voxels, the cloud stays inside the narrow-key range (its extent is unchanged)


def _shifted(pts, dx=0.0, dy=0.0, dz=0.0):
    pts = pts.copy()
    for a, v in (("x", dx), ("y", dy), ("z", dz)):
        pts[a] = (pts[a].astype(np.float64) + v).astype(np.float32)
    return pts


def cloud(name):
    from wildcat_slam_amd import synth

    if name == "lattice095":  # all three layers and the displaced root of the hash (stamps at 1.6e9 s, synth.T0)
        return synth.g2_lattice(60, m=40)[0], dict(voxel_size=0.95)
    if name == "q4":  # one patch per root: root and child surfels overlap
        return synth.g2_lattice(60, m=48, patches_per_root=1)[0], {}
    if name == "revisits3":  # three temporal clusters per node, small stamps
        parts = []
        for r in range(3):
            a = synth.g2_lattice(50, m=32, t_start=0.08 * r, duration=0.02)[0]
            a["x"] += np.float32(0.0005 * r)
            parts.append(a)
        return synth.concat_points(*parts), {}
    if name == "room":  # layer-0 planes, many clusters per node, exactly planar scan-line clusters
        return synth.g1_room(60_000, seed=synth.SEED + 3), {}
    if name == "epoch":  # epoch stamps that are no short binary fractions, over another sweep length
        return synth.g2_lattice(60, m=40, t_start=1.6e9 + 0.123456789, duration=0.31)[0], dict(voxel_size=0.95)
    if name == "far":  # coordinates around 500 m: |c|^2 in the fall-back band, 2^-15 m between neighbouring floats
        return _shifted(synth.g2_lattice(60, m=40)[0], dx=FAR_SHIFT), dict(voxel_size=0.95)
    if name == "straddle":  # patches across the world planes x = 0 and y = 0: coordinates below 2^-8 m, the only ones finer than the 2^-32 m grid
        return _shifted(synth.g2_lattice(40, m=160, span=4, seed=synth.SEED + 5)[0], dx=0.2, dy=0.2), {}
    if name == "dense":  # 16 000 points in one layer-1 cell: second moments beyond 2^53 grid units, a cell over sixteen tiles
        return synth.g2_lattice(1, m=16000, patches_per_root=2, span=4, seed=synth.SEED + 6)[0], {}
    if name == "edges":  # cells and clusters of exactly 19, 20 and 21 points (n > min_points, n >= cluster_min_points)
        def thinned(seed, t_start):
            a = synth.g2_lattice(45, m=21, seed=seed, t_start=t_start, duration=0.02)[0]
            j, root = np.arange(len(a)) % 21, np.arange(len(a)) // (8 * 21)
            return a[j < 19 + root % 3]

        first = thinned(synth.SEED + 7, 0.0)  # ... revisited in full 0.08 s later: tested cells of 40 / 41 / 42 points, first cluster 19 / 20 / 21
        again = _shifted(synth.g2_lattice(45, m=21, seed=synth.SEED + 7, t_start=0.08, duration=0.02)[0], dx=0.0005)
        alone = thinned(synth.SEED + 8, 0.16)  # cells of 19 / 20 / 21 points: only the last is tested
        return synth.concat_points(first, again, alone), {}
    if name == "planar":  # patches flattened onto planes z = const: clusters that span a plane exactly, smallest eigenvalue 0
        pts = synth.g2_lattice(40, m=32, seed=synth.SEED + 9)[0]
        z = pts["z"].astype(np.float64)
        pts["z"] = ((np.floor(z / 0.8) + 0.5) * 0.8 + np.where(z - np.floor(z / 0.8) * 0.8 > 0.4, 0.2, -0.2)).astype(np.float32)
        return pts, {}
    raise KeyError(name)


_CACHE = {}


def reference(name, base_params):
    """(points, params, extract(points, params)) of a cloud, computed once per process; base_params: a fresh default wc_params"""
    if name not in _CACHE:
        pts, over = cloud(name)
        for k_, v in over.items():
            setattr(base_params, k_, v)
        _CACHE[name] = (pts, base_params, extract(pts, base_params))
    return _CACHE[name]


def bounds(ref, params):
    """the per-surfel error bounds of the default arithmetic, derived from the grids csrc/extract_fast.inc documents:
    covariance entry, centre coordinate (M, 3), smallest eigenvalue, normal"""
    vs = float(np.float32(params.voxel_size))
    ev = ref["ev"].astype(np.float64)
    b_cov = 2.0**-45 + 2 * 2.0**-33 * vs * ref["f"] + 16 * 2.0**-53 * (vs / 2) ** 2
    b_c = 2.0**-33 * ref["f"][:, None] + 4 * 2.0**-53 * np.maximum(np.abs(ref["center"].astype(np.float64)), vs)
    b_lam = 3 * b_cov + 32 * 2.0**-53 * ev[:, 2]
    b_n = (b_lam + 1e-12 * (np.abs(ev[:, 0]) + ev[:, 2])) / (ev[:, 1] - ev[:, 0])
    return dict(cov=b_cov, center=b_c, lam=b_lam, normal=b_n)
