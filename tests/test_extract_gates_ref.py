"""What tests/test_extract_gates_gpu.py assumes of the gate clouds (tests/extract_gates.py), asserted without a GPU: every case reaches the
site it is built for, its margin / band lies in its class, nothing else in its sweep is anywhere near a threshold, the CPU oracle's ids are
the longdouble reference's wherever the default path may decide itself (so the GPU test can take the oracle for the truth) - and
grid_moments, the default path's integer-grid arithmetic restated in Python integers, agrees with the reference's covariance within the
documented B_cov on the clouds of tests/extract_ref.py."""
import numpy as np
import pytest

import extract_gates as G
import extract_ref as X
import helpers


def _params(oracle, over):
    p = oracle.default_params()
    for k_, v in over.items():
        setattr(p, k_, v)
    return p


def test_the_defaults_the_cases_are_built_for(oracle):
    p = oracle.default_params()
    q = G._Params()
    for k_ in ("voxel_size", "planer_threshold", "min_plane_likeness", "min_points", "cluster_min_points", "cluster_gap", "max_layer"):
        assert float(getattr(p, k_)) == float(np.float32(getattr(q, k_)) if k_ in ("voxel_size", "planer_threshold") else getattr(q, k_)), k_
    assert [p.view_point[i] for i in range(3)] == list(q.view_point)


def test_the_classes_cover_every_site_and_gate():
    for gate, sites in (("lam0", ("root", "l1", "job")), ("like", ("root", "l1", "l2", "job"))):
        for site in sites:
            have = {(G.case(n)["cls"], np.sign(G.case(n)["margin"])) for n in G.CASES if n.startswith("%s-%s-" % (gate, site))}
            assert {("decide", 1), ("decide", -1), ("grey", 1), ("grey", -1)} <= have and any(c == "fall" for c, _ in have), (gate, site, have)
    for site in ("root", "l1", "l2"):
        for phase in ("adj", "skip"):
            have = {G.case(n)["ticks"] for n in G.CASES if n.startswith("gap-%s-%s-" % (site, phase))}
            assert {-16, -4, 4, 16} <= have


@pytest.mark.parametrize("name", G.CASES)
def test_case_reaches_its_site_in_its_class(oracle, name):
    c = G.case(name)
    pts, ref, S = c["points"], c["ref"], c["ref"]["stats"]
    assert np.all(np.diff(pts["time"]) >= 0) and 64 < len(pts) <= 4000
    xyz = np.stack([pts["x"], pts["y"], pts["z"]], 1).astype(np.float64)
    assert np.sqrt((xyz**2).sum(axis=1)).max() < 40.0
    margin = {kind: S[kind + "_margin"] for kind in ("node", "cluster")}
    band = {kind: S[kind + "_band"] for kind in ("node", "cluster")}
    site = set()
    if c["gate"] == "gap":
        # the site: a plane node of the layer with 42 points in two groups, cluster_gap + k ticks apart - the nearest pair of the sweep
        assert c["tick"] == G.tick_of(pts) and abs(c["delta"] - c["ticks"] * c["tick"]) <= 2.0**-55
        assert S["min_gap_dist"] == abs(c["delta"]) and abs(c["ticks"]) in (4, 16, 32)
        assert c["bins"][1] - c["bins"][0] == (2 if c["phase"] == "skip" else 1)
        at = ref["layer"] == c["layer"]
        assert sorted(ref["n"][at].tolist()) == ([21, 21] if c["delta"] > 0 else [42]), ref["n"]
        assert c["cls"] == ("fall" if abs(c["ticks"]) <= 4 else "decide")
        if name.startswith("gap-bridged"):  # the child splits, the root - a point of another child inside the gap - does not
            assert ref["n"][ref["layer"] == 0].tolist() == [43]
    else:
        assert 21 <= c["n"] <= 64
        site = set(c["rows"])
        assert site and all(S[kind + "_layer"][i] == c["layer"] and S[kind + "_n"][i] == c["n"] for kind, i in site)
        for kind, i in site:  # the gate the case is named for is the nearer one, at the distance the case states
            assert abs(margin[kind][i] - abs(c["margin"])) <= 1e-3 * abs(c["margin"]) + 2e-18 and c["other_gate"] > 1e3 * abs(c["margin"])
        print("\n%s: n %d, |c| %.1f m, margin %+.3e, band %.3e, the path's own bound %.3e: margin / band %.2f -> %s"
              % (name, c["n"], float(np.linalg.norm(c["centre"])), c["margin"], c["band"], c["bound"], abs(c["margin"]) / c["band"], c["cls"]))
        assert c["cls"] == G.classify(c["margin"], c["band"], c["bound"])
        if c["want"] in ("fall", "grey", "decide"):
            assert c["cls"] == c["want"]
        elif c["want"] == "origin":  # the grey zone where the band is narrowest: n <= 25 within 2 m of the origin
            assert c["cls"] == "grey" and c["n"] <= 25 and np.linalg.norm(c["centre"]) < 2.0
        elif c["want"] == "between":  # (double)0.01f < lambda_0 < 0.01: "not a plane"
            assert G.THR < G.THR + c["margin"] < 0.01 and min(c["margin"], 0.01 - G.THR - c["margin"]) > 1e-10
            assert not (ref["n"] == c["n"]).any()
        assert S["min_gap_dist"] >= 1e-3
    # every other node and cluster of the sweep decides 1e4 bands away from both thresholds
    for kind in ("node", "cluster"):
        for i in range(len(margin[kind])):
            assert (kind, i) in site or margin[kind][i] >= 1e4 * band[kind][i], (kind, i, margin[kind][i], band[kind][i])
    # where the default path may decide itself, the oracle is the truth: its ids are the reference's
    if c["cls"] != "fall":
        params = _params(oracle, c["over"])
        s, ids, st = oracle.extract_surfels(pts, params)
        assert len(ids) == len(ref["ids"]) and set(helpers.id_tuples(ids)) == set(helpers.id_tuples(ref["ids"]))
        if len(ids):
            helpers.check_surfels(ref["surfels"], ref["ids"], s, ids, tol=1e-6, t_tol=1e-5)


def test_adversarial_cluster_the_grid_and_the_exact_moments_disagree_outside_the_reference_noise():
    """the outcome of the search DESIGN.md 4.3 records: a cluster whose lambda_0 on the path's grids and whose exact lambda_0 lie on
    opposite sides of (double)0.01f, further from it than 16 x the reference's rounding noise (the band as it was) - and inside the band as
    it is, which adds the path's own grid error"""
    c = G.case("lam0-root-slab")
    p = c["cluster"]
    n, cm = len(p), p.astype(np.float64).mean(axis=0)
    old = 16.0 * np.sqrt(n) * ((cm * cm).sum() + 1.0) * 2.0**-53 + 1e-14  # the band as it was: 16 x the reference's noise
    exact, grid = c["margin"], c["grid_lam0"] - G.THR
    print("\nslab cluster: n %d, f %.2f, exact lambda_0 - thr %+.3e, on the grids %+.3e, the band as it was %.3e (margin / band %.1f), the band %.3e"
          % (n, c["f"], exact, grid, old, exact / old, c["band"]))
    assert exact > 16 * old and grid < -16 * old
    assert abs(exact) + c["bound"] <= c["band"] and c["cls"] == "fall"  # the band as it is: the path must hand this sweep over
    assert abs(grid - exact) <= c["bound"]  # the documented bound holds: it is the band that forgot it


@pytest.mark.parametrize("name", X.CLOUDS)
def test_grid_moments_against_the_reference_covariance(oracle, name):
    pts, params, ref = X.reference(name, oracle.default_params())
    B = X.bounds(ref, params)
    vs = float(np.float32(params.voxel_size))
    M = len(ref["ids"])
    pick = set(np.random.default_rng(11).choice(M, size=min(M, 10), replace=False).tolist()) | {int(np.argmax(ref["f"])), int(np.argmin(ref["sigma2"]))}
    xyz = np.stack([pts["x"], pts["y"], pts["z"]], 1).astype(np.float64)
    worst = 0.0
    for i in sorted(pick):
        mem = ref["members"][i][:4000]  # (a whole 16 000-point cell in Python integers is seconds: its first 4 000 points, against their own moments)
        cc = (0.5 + np.array([ref["ids"][a][i] for a in ("kx", "ky", "kz")], np.float64)) * vs
        g = G.grid_moments(xyz[mem], cc)
        if len(mem) == ref["n"][i]:
            cov, b = ref["cov"][i], B["cov"][i]
        else:
            d = xyz[mem].astype(X.LD) - cc.astype(X.LD)
            cov = X._pca(d, np.zeros(len(mem)), np.zeros(len(mem), bool), np.array([0]), np.array([len(mem)]), cc[None, :])["cov"][0]
            b = 2.0**-45 + 2 * 2.0**-33 * vs + 16 * 2.0**-53 * (vs / 2) ** 2
        worst = max(worst, float(np.abs(g["cov"].astype(X.LD) - cov).max()) / b)
    print("\n%s: grid_moments against the reference covariance, worst error / B_cov over %d clusters: %.3g" % (name, len(pick), worst))
    assert worst <= 1.0
