"""The plain restatement of the matcher (tests/match_ref.py) against the CPU oracle, and the gate scenes of tests/match_gates.py: every
case live, every case on the side it was built for.  No GPU.

Measured here (glibc's acos, the libm the oracle calls): c* is the smallest double whose acos is <= ang_max; the gap
acos(c* + j ulp) - ang_max, in ulp of ang_max, is
    ang_max   j = -4      -3      -2      -1       0      +1      +2      +3      +4
    0.5 deg   +27952  +20618  +13284   +5950   -1384   -8718  -16051  -23385  -30719      c* = 0.9999619230641713
    5 deg       +357    +265    +173     +81     -10    -102    -194    -286    -377      c* = 0.9961946980917455
    30 deg        +7      +5      +3      +1      -1      -3      -5      -7      -9      c* = 0.8660254037844387
(test_the_hosts_acos_next_to_the_threshold prints them).  At 0.5 and 5 deg an acos that is a few ulp off decides c* - 1 ulp and c* like
the host's; at 30 deg the two lie ONE ulp of the angle on either side of ang_max, and an acos that rounds the other way there flips
the gate.  acos is monotone over +-2000 ulp around every c*: match_gates.c_star asserts that."""
import math

import numpy as np
import pytest

import match_gates as G
import match_ref as M
from wildcat_slam_amd import records as R
from wildcat_slam_amd import synth

KS = (1, 3, 10, 16)
SCENE_IDS = [(n, s) for n in sorted(G.SCENES) for s in (True, False)]


def _wc(oracle, P):
    return M.to_wc_params(P, oracle.default_params())


def _equal_to_oracle(oracle, sc, P, ks):
    """pairs and lists of the restatement against oracle.match / oracle.knn6, byte for byte, at every k of ks; -> {k: result}"""
    q, qp, t, tp, same = sc["q_surf"], sc["q_pose"], sc["t_surf"], sc["t_pose"], sc["same_set"]
    kmax = max(ks)
    Pm = M.params(**dict(vars(P), knn_k=kmax))
    ft = M.features(t, tp, Pm)
    fq = ft if same else M.features(q, qp, Pm)
    lists = M.knn(ft, fq, kmax)
    out = {}
    for k in ks:
        Pk = M.params(**dict(vars(P), knn_k=k))
        ref = M.match(q, qp, t, tp, same, Pk, lists=lists)
        assert ref["rc"] == 0
        oidx, od2 = oracle.knn6(ft, fq, k)
        assert ref["idx"].tobytes() == oidx.tobytes() and ref["d2"].tobytes() == od2.tobytes(), (sc.get("name"), k, "lists")
        opairs = oracle.match(q, qp, t, tp, same, _wc(oracle, Pk))
        assert ref["pairs"].tobytes() == opairs.tobytes(), (sc.get("name"), k, "pairs")
        out[k] = ref
    return out


def _random_scene(rng, n, extent, t0=0.0):
    s = np.zeros(n, R.SURFEL)
    s["center"] = rng.uniform(-extent / 2, extent / 2, size=(n, 3))
    nrm = rng.normal(size=(n, 3))
    s["normal"] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    s["t"] = t0 + np.sort(rng.uniform(0, 5, size=n))
    p = np.zeros(n, R.POSE)
    p["quat"][:, 0] = 1.0
    return s, p


@pytest.mark.parametrize("same_set", [True, False])
def test_restatement_equals_the_oracle_on_the_window_scenes(oracle, same_set):
    """synth.surfel_window with its real poses (qrot with general quaternions), both kinds of search, k of 1, 3, 10, 16; with the gates as
    they are and with gates that cut through the lists"""
    w = synth.surfel_window(3, 90, seed=31, fixed_patches=70)
    rng = np.random.default_rng(77)
    w["surf"]["normal"] += rng.normal(scale=0.03, size=w["surf"]["normal"].shape)
    w["surf"]["center"] += rng.normal(scale=0.02, size=w["surf"]["center"].shape)
    sc = dict(name="window", same_set=same_set, q_surf=w["surf"], q_pose=w["pose"], t_surf=w["surf"] if same_set else w["fix_surf"],
              t_pose=w["pose"] if same_set else w["fix_pose"])
    dt = float(np.ptp(w["surf"]["t"]))
    n_pairs = []
    for over in (dict(), dict(time_diff_min=0.45 * dt), dict(surfel_dist_max=0.004), dict(angular_scale=1.0 * G.DEG, center_scale=0.5)):
        res = _equal_to_oracle(oracle, sc, M.params(**over), KS)
        n_pairs.append(len(res[10]["pairs"]))
    assert n_pairs[0] > 0.3 * len(w["surf"]) * (1 if same_set else 0.3) and min(n_pairs) < n_pairs[0]


def test_restatement_equals_the_oracle_on_random_scenes(oracle):
    """the random scenes of tests/test_match_gpu.py at small size: a sparse wide cube, queries outside the targets' box, fewer targets than k"""
    rng = np.random.default_rng(78)
    s, p = _random_scene(rng, 400, 600.0)
    _equal_to_oracle(oracle, dict(name="sparse", same_set=True, q_surf=s, q_pose=p, t_surf=s, t_pose=p), M.params(), KS)
    t, tp = _random_scene(rng, 500, 6.0)
    q, qp = _random_scene(rng, 200, 18.0, t0=10.0)
    _equal_to_oracle(oracle, dict(name="outside", same_set=False, q_surf=q, q_pose=qp, t_surf=t, t_pose=tp), M.params(), KS)
    w = synth.surfel_window(2, 3, seed=4)
    res = _equal_to_oracle(oracle, dict(name="few", same_set=True, q_surf=w["surf"], q_pose=w["pose"], t_surf=w["surf"], t_pose=w["pose"]), M.params(), KS)
    assert (res[10]["idx"][:, 6:] == 0).all() and (res[10]["d2"][:, 6:] == 0).all()  # Q10: the zero tail


@pytest.mark.parametrize("name,same_set", SCENE_IDS)
def test_gate_scenes_equal_the_oracle_and_every_case_is_live(oracle, name, same_set):
    """every scene of match_gates.py and its mirror: the restatement is the oracle byte for byte (k = 1 and 10); no list of a cluster's Q,
    N1 or N2 leaves the cluster; N1 is Q's nearest candidate and N2 the next, N1's other two gates and all of N2's pass; the case's gate
    decides as the case was built to; and with the operand mirrored across the threshold Q is paired differently - 100 % of the cases"""
    P = G.scene_params(name)
    sc, mi = G.scene(name, same_set), G.scene(name, same_set, mirror=True)
    ref = _equal_to_oracle(oracle, sc, P, (1, 10))[10]
    mref = _equal_to_oracle(oracle, mi, P, (1, 10))[10]
    meas, mmeas = G.measure(sc, ref, P), G.measure(mi, mref, P)
    self_pos = 1 if same_set else 0
    live = 0
    for c, mc, m, mm in zip(sc["cases"], mi["cases"], meas, mmeas):
        for r_ in (ref, mref):
            for who in ("q", "n1", "n2"):
                if who == "q" or same_set:
                    assert set(r_["idx"][c[who]].tolist()) <= set(c["members"]), (c["id"], who, "a list leaves the cluster")
        assert m["pos"] == self_pos and m["n2_pos"] == self_pos + 1, (c["id"], m)
        assert m["others"] and m["n2_passes"] and mm["others"] and mm["n2_passes"], (c["id"], m, mm)
        want = _built_side(c)
        assert m["passed"] == want and mm["passed"] == (not want), (c["id"], m, mm)
        if c["kind"] == "ulp" and c["gate"] != "time":
            assert m["ulp"] == c["value"], (c["id"], m)  # the operand IS the chosen number
        if c["kind"] == "ulp" and c["gate"] == "time":
            j, base = c["value"]
            assert m["ulp"] == j * (1.0 if base == 0.0 else G.STAMP_ULP / G.ulp(P.time_diff_min)), (c["id"], m)
        if c["gate"] == "angle" and c["kind"] == "ulp":
            assert m["ulp_ang"] == G.c_star(P.angular_scale)[1][c["value"]]
        assert G.pairs_of(ref["pairs"], sc, c) != G.pairs_of(mref["pairs"], mi, mc), (c["id"], "not live")
        live += 1
    assert live == len(sc["cases"]) >= (7 if G.SCENES[name][4] == "S" else 40)


def _built_side(c):
    gate, kind, v = c["gate"], c["kind"], c["value"]
    if kind == "ulp":
        return v <= 0 if gate == "plane" else (v[0] if gate == "time" else v) >= 0
    if kind == "rel":
        return v < 0
    if kind == "nan":
        return True
    return v[0] == "pass"


def test_the_hosts_acos_next_to_the_threshold():
    """c* by bisection for the three angles of the scenes: acos is monotone around it (asserted inside c_star), c* passes and c* - 1 ulp
    does not, and the gaps are the ones this module's docstring records"""
    for deg in (0.5, 5.0, 30.0):
        ang = deg * G.DEG
        c, gaps = G.c_star(ang)
        assert math.acos(c) <= ang < math.acos(G.step(c, -1))
        assert all(gaps[j] <= 0 for j in range(0, 5)) and all(gaps[j] > 0 for j in range(-4, 0))
        assert abs(c - math.cos(ang)) <= 2 * G.ulp(c)
        print("%4.1f deg: c* = %r, gaps [ulp of ang_max] %s" % (deg, c, " ".join("%+.1f" % gaps[j] for j in range(-4, 5))))


def test_scenes_reach_into_the_early_walks_margins():
    """The early walk (match_tree.inc) accepts a candidate on dn as as >= cos_acc and fabs(dp) as cs <= plane_acc - 1e-9 qmax cs, formed
    from the features.  Restated (match_ref.early_operands): among the cases whose gate REJECTS N1 there are some that the walk would
    accept if cos_acc were cos(ang_max), and some that it would accept if the 1e-9 qmax cs term were missing - only the margins keep
    those walks from being bounded by a candidate the gate rejects, which would lose Q's pair with N2.  With the margins as they are
    no rejected N1 is accepted."""
    thin_cos = thin_plane = accepted = 0
    for name in sorted(G.SCENES):
        P = G.scene_params(name)
        cos_acc, plane_acc = M.early_margins(P)
        sc = G.scene(name, False)
        ref = M.match(sc["q_surf"], sc["q_pose"], sc["t_surf"], sc["t_pose"], False, P)
        fq, ft = M.features(sc["q_surf"], sc["q_pose"], P), M.features(sc["t_surf"], sc["t_pose"], P)
        for c, m in zip(sc["cases"], G.measure(sc, ref, P)):
            if m["passed"] or c["gate"] == "time":
                continue
            cs_, pl_, qmax = M.early_operands(fq[c["q"]], ft[c["n1"] : c["n1"] + 1], P)
            plane_ok = pl_[0] <= plane_acc - 1e-9 * qmax * P.center_scale
            accepted += int(cs_[0] >= cos_acc and plane_ok)
            thin_cos += int(cs_[0] >= math.cos(P.angular_scale) and pl_[0] <= P.surfel_dist_max - 1e-9 * qmax * P.center_scale and c["gate"] == "angle")
            thin_plane += int(cs_[0] >= cos_acc and pl_[0] <= plane_acc and c["gate"] == "plane")
    print("rejected N1 the early walk would accept: margins as they are %d, cos_acc = cos(ang_max) %d, without the qmax term %d" % (accepted, thin_cos, thin_plane))
    assert accepted == 0 and thin_cos >= 3 and thin_plane >= 3


@pytest.mark.parametrize("kind", ["block", "few"])
@pytest.mark.parametrize("same_set", [True, False])
def test_tie_scenes_equal_the_oracle(oracle, kind, same_set):
    """the tie scenes of the GPU tests: the oracle's pruning is <= and its Best::push orders equal distances by index, so its lists and
    pairs are the brute-force ones; and the scenes do what they are for: lists with equal distances, the time gate cutting through them"""
    sc = G.tie_scene(kind, same_set)
    res = _equal_to_oracle(oracle, sc, sc["P"], KS)
    r = res[10]
    nt = len(sc["t_surf"])
    valid = r["d2"][:, : min(10, nt)]
    tied = (np.diff(valid, axis=1) == 0).any(axis=1)
    assert tied.mean() > 0.5
    cut = r["passed"][:, : min(10, nt), 0]
    assert 0.25 < cut[tied].mean() < 0.75  # about half of the tied candidates fail the time gate
    assert len(r["pairs"]) > 0
