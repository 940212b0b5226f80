"""tests/extract_ref.py - the longdouble reference the default extraction path is measured against - is itself held, without a GPU:
against the CPU oracle (same ids, geometry within the oracle's own 1e-6), against exact rational arithmetic (its moments and eigenpairs
must be at least 1000 x finer than the tightest bound tests/test_extract_precision_gpu.py asserts), and for what those GPU tests rely on
in every cloud: the layers and cluster counts reached, gates far outside the band in which the default path hands a sweep to the exact
arithmetic, no stamp gap at the clustering threshold."""
import os
from fractions import Fraction

import numpy as np
import pytest

import extract_ref as X
import helpers
from wildcat_slam_amd import records as R

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# surfels by layer, temporal clusters seen, clusters rejected by the gates
EXPECT = {
    "lattice095": ((170, 355, 26), 551, 0),
    "q4": ((60, 60, 0), 120, 0),
    "revisits3": ((0, 1200, 0), 1200, 0),
    "room": ((416, 0, 0), 6832, 2),
    "epoch": ((170, 355, 26), 551, 0),
    "far": ((170, 355, 26), 551, 0),
    "straddle": ((30, 449, 204), 780, 78),
    "dense": ((1, 2, 0), 3, 0),
    "edges": ((0, 720, 0), 840, 0),
    "planar": ((0, 227, 2), 229, 0),
}


def _against_oracle(oracle, pts, params, ref):
    s, ids, st = oracle.extract_surfels(pts, params)
    assert len(ref["ids"]) == len(ids) == st.surfels
    assert set(helpers.id_tuples(ref["ids"])) == set(helpers.id_tuples(ids))
    info = helpers.check_surfels(ref["surfels"], ref["ids"], s, ids, tol=1e-6, t_tol=1e-5)
    S = ref["stats"]
    assert S["root_voxels"] == st.root_voxels
    assert S["nodes_tested"] == list(st.nodes_tested)[:3] and S["nodes_plane"] == list(st.nodes_plane)[:3]
    assert (S["clusters_total"], S["clusters_rejected"]) == (st.clusters_total, st.clusters_rejected)
    assert abs(S["min_gate_margin"] - st.min_gate_margin) <= 1e-6 * st.min_gate_margin + 1e-9  # (the oracle's margin carries its sums' noise)
    return info


def test_reference_equals_oracle_on_the_golden_cloud(oracle):
    z = np.load(os.path.join(G, "extract_small.npz"))
    pts = np.ascontiguousarray(z["points"]).view(R.POINT).reshape(-1)
    params = oracle.default_params()
    ref = X.extract(pts, params)
    info = _against_oracle(oracle, pts, params, ref)
    assert info["n"] > 1000
    # ... and the recorded surfels of the fixture themselves
    helpers.check_surfels(ref["surfels"], ref["ids"], z["surfels"].view(R.SURFEL).reshape(-1), z["ids"].view(R.SURFEL_ID).reshape(-1), tol=1e-6, t_tol=1e-5)


@pytest.mark.parametrize("name", X.CLOUDS)
def test_reference_equals_oracle_and_the_cloud_reaches_what_it_is_there_for(oracle, name):
    pts, params, ref = X.reference(name, oracle.default_params())
    assert np.all(np.diff(pts["time"]) >= 0) and len(pts) <= 60_000
    _against_oracle(oracle, pts, params, ref)
    S = ref["stats"]
    layers, clusters, rejected = EXPECT[name]
    assert tuple(np.bincount(ref["layer"], minlength=3)) == layers
    assert (S["clusters_total"], S["clusters_rejected"]) == (clusters, rejected)
    # the output order: own stamps, ties by id
    keys = list(zip(ref["surfels"]["t"].tolist(), helpers.id_tuples(ref["ids"])))
    assert keys == sorted(keys)
    # every gate at least 1e4 x further from its threshold than the band in which fx_pca would hand the sweep to the exact arithmetic:
    # the GPU tests then measure the default path (they assert it, too), and no decision hangs on either side's rounding
    margin = np.concatenate([S["node_margin"], S["cluster_margin"]])
    band = np.concatenate([S["node_band"], S["cluster_band"]])
    print("\n%s: smallest gate margin %.3g, widest fall-back band %.3g, smallest margin / band %.3g, stamp gap nearest to cluster_gap at %.3g s"
          % (name, margin.min(), band.max(), (margin / band).min(), S["min_gap_dist"]))
    assert np.all(margin >= 1e4 * band)
    assert S["min_gap_dist"] >= 1e-6
    if name == "straddle":  # coordinates finer than the 2^-32 m grid are in play, in surfels on both world planes
        m = np.stack([pts["x"], pts["y"]], 1)
        assert (ref["f"] > 0).sum() >= 50 and all((np.abs(m[:, a]) < 2.0**-8).sum() > 100 for a in (0, 1))
    if name == "dense":  # the sums of squares of a 16 000-point cell about its voxel centre pass 2^53 units of 2^-44 m^2
        assert sorted(ref["n"].tolist()) == [16000, 16000, 32000]
        p, vs = np.stack([pts["x"], pts["y"], pts["z"]], 1).astype(np.float64), float(np.float32(params.voxel_size))
        for i in np.flatnonzero(ref["n"] == 16000):
            q = p[ref["members"][i]]
            q = q - (0.5 + np.floor(q / vs)) * vs
            assert ((q * q).sum(axis=0) * 2.0**44).max() > 2.0**53
    if name == "edges":
        sizes = np.bincount(S["cluster_sizes_all"], minlength=23)
        assert sizes[19] == 120 and sizes[20] == 120 and sizes[21] == 600 and sizes.sum() == 840
        assert np.bincount(ref["n"], minlength=22)[[19, 20, 21]].tolist() == [0, 120, 600]  # n >= cluster_min_points
        lone = S["node_n"][S["node_layer"] == 1]
        assert (lone == 21).sum() == 120 and (lone == 20).sum() == 0 and (lone == 19).sum() == 0  # n > min_points
    if name == "room":  # many temporal clusters per node (every pass of a beam), coordinates below 2^-8 m on the floor plane z = 0
        assert S["clusters_total"] > 5 * sum(S["nodes_plane"]) and (ref["f"] > 0).any()
    if name == "planar":  # every cluster spans a plane EXACTLY: the smallest eigenvalue is zero, its root is where a NaN can appear
        assert np.all(ref["sigma2"] == 0) and len(ref["ids"]) == 229
    if name == "revisits3":
        assert np.all(((ref["ids"]["node"] >> 8).astype(np.int64)) <= 2) and len({int(v) >> 8 for v in ref["ids"]["node"]}) == 3


def _exact_moments(points, members):
    """centre, population covariance and stamp mean of the points `members` in exact rational arithmetic: the coordinates are floats,
    so scaled by a power of two they are integers, and the sums are Python integers"""
    cols = [[float(points[a][i]).as_integer_ratio() for i in members] for a in ("x", "y", "z", "time")]
    n = len(members)
    ints, dens = [], []
    for col in cols:
        K = max(d for _, d in col)
        ints.append([num * (K // d) for num, d in col])
        dens.append(K)
    s1 = [sum(v) for v in ints]
    c = [Fraction(s1[a], n * dens[a]) for a in range(3)]
    cov = [[Fraction(n * sum(x * y for x, y in zip(ints[a], ints[b])) - s1[a] * s1[b], n * n * dens[a] * dens[b]) for b in range(3)] for a in range(3)]
    return c, cov, Fraction(s1[3], n * dens[3])


@pytest.mark.parametrize("name", X.CLOUDS)
def test_reference_against_exact_rational_arithmetic(oracle, name):
    """about 50 sampled clusters per cloud (the smallest eigenvalue's extremes, the largest cluster and the largest f among them): the
    longdouble centre, covariance, stamp and eigenpairs (|| C v - lambda v ||, |v . v - 1|: C exact, the arithmetic in Fraction) against
    1/1000 of the bounds the GPU tests assert FOR THAT CLUSTER (extract_ref.bounds; stamp 3e-7 s; unit length 8 x 2^-53) - every figure
    below 1 means the reference's own error is invisible in those tests."""
    pts, params, ref = X.reference(name, oracle.default_params())
    B = X.bounds(ref, params)
    M = len(ref["ids"])
    rng = np.random.default_rng(5)
    pick = set(rng.choice(M, size=min(M, 46), replace=False).tolist())
    pick |= {int(np.argmin(ref["sigma2"])), int(np.argmax(ref["sigma2"])), int(np.argmax(ref["n"])), int(np.argmax(ref["f"]))}
    F = X.ld_to_fraction
    worst = dict(center=0.0, cov=0.0, t=0.0, eig=0.0, normal=0.0, unit=0.0)
    for i in sorted(pick):
        c, cov, tm = _exact_moments(pts, ref["members"][i])
        assert len(ref["members"][i]) == ref["n"][i]
        for a in range(3):
            worst["center"] = max(worst["center"], float(abs(F(ref["center"][i, a]) - c[a])) / B["center"][i, a])
            for b in range(3):
                worst["cov"] = max(worst["cov"], float(abs(F(ref["cov"][i, a, b]) - cov[a][b])) / B["cov"][i])
        worst["t"] = max(worst["t"], float(abs(F(ref["t"][i]) - tm)) / 3e-7)
        V = ref["evecs"][i]
        assert np.array_equal(np.abs(V[:, 0]), np.abs(ref["normal"][i]))
        for k in range(3):
            v = [F(V[a, k]) for a in range(3)]
            lam = F(ref["ev"][i, k])
            r = [sum(cov[a][b] * v[b] for b in range(3)) - lam * v[a] for a in range(3)]
            res = float(sum(x * x for x in r)) ** 0.5
            worst["eig"] = max(worst["eig"], res / B["lam"][i])
            worst["unit"] = max(worst["unit"], float(abs(sum(x * x for x in v) - 1)) / 2 / (8 * 2.0**-53))
            if k == 0:  # the normal's distance from the exact eigenvector is at most residual / gap
                gap = float(ref["ev"][i, 1] - ref["ev"][i, 0])
                worst["normal"] = max(worst["normal"], res / gap / B["normal"][i])
    print("\n%s: reference error / (GPU bound / 1000), worst of %d clusters: " % (name, len(pick)) + ", ".join("%s %.3g" % (k, 1000 * v) for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1e-3, (k, v)


def test_batched_jacobi_against_numpy_and_its_own_residual():
    rng = np.random.default_rng(3)
    q, _ = np.linalg.qr(rng.normal(size=(200, 3, 3)))
    lam = np.sort(10 ** rng.uniform(-14, 0, size=(200, 3)), axis=1)
    A = np.einsum("mij,mj,mkj->mik", q, lam, q)
    A = (A + A.transpose(0, 2, 1)) / 2
    ev, V = X.jacobi_eigh(A)
    assert np.all(np.diff(ev, axis=1) >= 0)
    res = np.abs(np.einsum("mij,mjk->mik", A.astype(X.LD), V) - V * ev[:, None, :]).max(axis=(1, 2))
    assert np.all(res <= 8 * 2.0**-63 * lam[:, 2])
    assert np.abs(np.einsum("mji,mjk->mik", V, V) - np.eye(3)).max() <= 8 * 2.0**-63
    assert np.all(np.abs(ev.astype(np.float64) - np.linalg.eigvalsh(A)) <= 1e-13 * lam[:, 2:])  # (LAPACK in fp64 is the coarse side here)
    # degenerate inputs: the zero matrix, a diagonal one, equal eigenvalues - finite, orthonormal, in order
    ev, V = X.jacobi_eigh(np.array([np.zeros((3, 3)), np.diag([3.0, 1.0, 2.0]), np.eye(3)]))
    assert np.array_equal(ev.astype(np.float64), [[0, 0, 0], [1, 2, 3], [1, 1, 1]]) and np.isfinite(V.astype(np.float64)).all()
