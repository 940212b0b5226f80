"""The matcher's gates at their thresholds, its early bound on ties, its state between calls and its failure returns, on the GPU,
against the plain restatement (tests/match_ref.py, held to the oracle without a GPU in tests/test_match_ref.py).

Scenes: tests/match_gates.py.  The final gates of csrc/match_tree.inc promise the reference's decision bit for bit - with the device's
acos next to ang_max, where one ulp of the cosine is 1 ulp of the angle at 30 deg and 7 000 at 0.5 deg - and the early walk (no lists
asked for) promises never to be bounded by a candidate those gates reject: the scenes put operands on, next to and a few 1e-10 from
the thresholds, and inside the early acceptance's margins.

Found with these tests: with the device's acos in the angle gate the decision differed from the reference's at ang_max = 60, 90 and
100 deg (cosines one to three doubles from the threshold) - the gate now compares the cosine with a threshold found on the host
(csrc/match.hip: match_cos_gate)."""
import ctypes as C

import numpy as np
import pytest

import match_gates as G
import match_ref as M
from wildcat_slam_amd import lib
from wildcat_slam_amd import records as R
from wildcat_slam_amd import synth

pytestmark = pytest.mark.gpu

KS = (1, 3, 10, 16)
_REF = {}


def _ref(sc, P, ks):
    """the restatement's results of a scene at every k of ks (computed once per scene: the lists at the largest k, prefixes below)"""
    key = (sc["name"], sc["same_set"], tuple(ks))
    if key not in _REF:
        q, qp, t, tp, same = sc["q_surf"], sc["q_pose"], sc["t_surf"], sc["t_pose"], sc["same_set"]
        Pm = M.params(**dict(vars(P), knn_k=max(ks)))
        ft = M.features(t, tp, Pm)
        lists = M.knn(ft, ft if same else M.features(q, qp, Pm), max(ks))
        _REF[key] = {k: M.match(q, qp, t, tp, same, M.params(**dict(vars(P), knn_k=k)), lists=lists) for k in ks}
    return _REF[key]


def _set(gpu, oracle, P, k):
    Pk = M.params(**dict(vars(P), knn_k=k))
    wp = M.to_wc_params(Pk, oracle.default_params())
    gpu.set_params(wp)
    return wp


def _run(ctx, sc, plain):
    """-> (pairs, idx, d2) - idx, d2 None for the early walk (no lists asked for)"""
    r = ctx.match(sc["q_surf"], sc["q_pose"], sc["t_surf"], sc["t_pose"], sc["same_set"], want_knn=plain)
    return r if plain else (r, None, None)


def _report(sc, got, ref, P):
    """the cases whose Q the GPU paired otherwise, one line each: gate, offset, operand's distance from the threshold, who took whom"""
    lines = []
    for c, m in zip(sc["cases"], G.measure(sc, ref, P) if ref["idx"].shape[1] >= 3 else [None] * len(sc["cases"])):
        if G.pairs_of(got, sc, c) != G.pairs_of(ref["pairs"], sc, c):
            lines.append(G.describe(sc, c, got, ref["pairs"]) + ("" if m is None else "  [reference: gate %s, operand %+.3g ulp from the threshold]" % ("passes" if m["passed"] else "rejects", m["ulp"])))
    if not lines and sc["same_set"]:  # (one set: N1, N2 and the others of a cluster are queries too - there the case's operand decides for them as well)
        def among(pairs, mem):
            return sorted((int(a), int(b)) for a, b in zip(pairs["first"], pairs["second"]) if a in mem or b in mem)

        for c in sc["cases"]:
            mem = set(c["members"])
            g, r = among(got, mem), among(ref["pairs"], mem)
            if g != r:
                lines.append("%s (Q %d, N1 %d, N2 %d): pairs in the cluster: GPU only %s, the reference only %s" % (c["id"], c["q"], c["n1"], c["n2"], sorted(set(g) - set(r)), sorted(set(r) - set(g))))
    return "\n".join(lines[:40]) or "(the differing pairs belong to no cluster)"


@pytest.mark.parametrize("same_set", [True, False])
@pytest.mark.parametrize("name", sorted(G.SCENES))
def test_gates_at_their_thresholds(gpu, oracle, name, same_set):
    """every scene of match_gates.py, early walk and plain walk, k = 1 and 10: the pair list is the restatement's and the oracle's byte for
    byte, the plain walk's tables are the restatement's"""
    P = G.scene_params(name)
    sc = G.scene(name, same_set)
    refs = _ref(sc, P, (1, 10))
    try:
        for k in (1, 10):
            wp = _set(gpu, oracle, P, k)
            ref = refs[k]
            assert ref["rc"] == 0
            opairs = oracle.match(sc["q_surf"], sc["q_pose"], sc["t_surf"], sc["t_pose"], same_set, wp)
            assert ref["pairs"].tobytes() == opairs.tobytes()
            for plain in (False, True):
                pairs, idx, d2 = _run(gpu, sc, plain)
                walk = "plain walk" if plain else "early walk"
                assert pairs.tobytes() == ref["pairs"].tobytes(), "%s %s k=%d, %s:\n%s" % (name, "same set" if same_set else "two sets", k, walk, _report(sc, pairs, ref, P))
                if plain:
                    assert np.array_equal(idx.astype(np.int64), ref["idx"].astype(np.int64)) and d2.tobytes() == ref["d2"].tobytes(), (name, k, "tables")
    finally:
        gpu.set_params(oracle.default_params())


@pytest.mark.parametrize("same_set", [True, False])
@pytest.mark.parametrize("kind", ["block", "few"])
def test_ties_under_both_walks(gpu, oracle, kind, same_set):
    """exactly equal feature distances (a 0.25 m lattice, normals along the axes, 1 500 coincident surfels among 3 000; seven targets for
    k = 10 and 16) with the time gate failing about half of every tied group: the early walk orders ties against its bound by
    (distance, index) and takes the nearest accepted point of a first full chunk by the same order - pairs of both walks and the plain
    walk's index tables are the restatement's at k = 1, 3, 10, 16"""
    sc = G.tie_scene(kind, same_set)
    refs = _ref(sc, sc["P"], KS)
    try:
        for k in KS:
            _set(gpu, oracle, sc["P"], k)
            ref = refs[k]
            for plain in (False, True):
                pairs, idx, d2 = _run(gpu, sc, plain)
                assert pairs.tobytes() == ref["pairs"].tobytes(), (kind, same_set, k, "plain walk" if plain else "early walk", _first_difference(pairs, ref["pairs"]))
                if plain:
                    assert np.array_equal(idx.astype(np.int64), ref["idx"].astype(np.int64)) and d2.tobytes() == ref["d2"].tobytes(), (kind, same_set, k, "tables")
    finally:
        gpu.set_params(oracle.default_params())


@pytest.mark.parametrize("ang", [3.2, -0.1])
def test_angle_gate_outside_zero_to_pi(gpu, oracle, ang):
    """angular_scale is a parameter: at or above pi no angle is larger (the gate rejects nothing), below zero every angle is (it rejects
    every dot product of [-1, 1]; one outside has a NaN angle and passes).  The gate decides on the cosine (match.hip: match_cos_gate):
    both of its ends, against the restatement and the oracle."""
    w = synth.surfel_window(3, 100, seed=12, fixed_patches=80)
    scenes = [dict(name="window", same_set=True, q_surf=w["surf"], q_pose=w["pose"], t_surf=w["surf"], t_pose=w["pose"]),
              dict(name="window", same_set=False, q_surf=w["surf"], q_pose=w["pose"], t_surf=w["fix_surf"], t_pose=w["fix_pose"]),
              G.tie_scene("block", False)]
    try:
        for sc in scenes:
            P = M.params(**dict(vars(sc.get("P", M.params())), knn_k=10, angular_scale=ang))
            wp = _set(gpu, oracle, P, 10)
            ref = M.match(sc["q_surf"], sc["q_pose"], sc["t_surf"], sc["t_pose"], sc["same_set"], P)
            assert ref["rc"] == 0 and ref["pairs"].tobytes() == oracle.match(sc["q_surf"], sc["q_pose"], sc["t_surf"], sc["t_pose"], sc["same_set"], wp).tobytes()
            assert ref["passed"][:, :, 1].all() if ang > 3.15 else not ref["passed"][:, :, 1][np.abs(ref["dot"]) <= 1.0].any()
            for plain in (False, True):
                pairs, idx, d2 = _run(gpu, sc, plain)
                assert pairs.tobytes() == ref["pairs"].tobytes(), (sc["name"], sc["same_set"], ang, plain, _first_difference(pairs, ref["pairs"]))
    finally:
        gpu.set_params(oracle.default_params())


def _first_difference(got, ref):
    n = min(len(got), len(ref))
    d = np.nonzero((got["first"][:n] != ref["first"][:n]) | (got["second"][:n] != ref["second"][:n]))[0]
    if len(d) == 0:
        return "%d pairs, the reference %d" % (len(got), len(ref))
    i = int(d[0])
    return "pair %d: GPU %s, reference %s (%d pairs, the reference %d)" % (i, tuple(got[i]), tuple(ref[i]), len(got), len(ref))


def test_state_between_calls(oracle):
    """eight calls on ONE context, large then small (3 000 / 900 surfels, then 7 / 5), k = 16 then 1, same set and two sets, early and
    plain walk in turn: every call returns the restatement's pairs.  The early walk writes a query's gated planes only up to the accepted
    entry, and every buffer is as large as the largest call left it - a stale word of the larger call must never be read."""
    ctx = lib.Context(0)
    try:
        plan = [("block", True, 16, False), ("few", False, 1, True), ("block", False, 16, True), ("few", True, 1, False),
                ("block", True, 16, True), ("few", False, 1, False), ("block", False, 16, False), ("few", True, 1, True)]
        for n_call, (kind, same_set, k, plain) in enumerate(plan):
            sc = G.tie_scene(kind, same_set)
            ref = _ref(sc, sc["P"], KS)[k]
            _set(ctx, oracle, sc["P"], k)
            pairs, idx, d2 = _run(ctx, sc, plain)
            assert pairs.tobytes() == ref["pairs"].tobytes(), (n_call, kind, same_set, k, plain, _first_difference(pairs, ref["pairs"]))
            if plain:
                assert np.array_equal(idx.astype(np.int64), ref["idx"].astype(np.int64)) and d2.tobytes() == ref["d2"].tobytes(), (n_call, "tables")
    finally:
        ctx.close()


def _raw_match(ctx, q_surf, q_pose, t_surf, t_pose, cap):
    """wc_match on two sets with a pair capacity of its own -> (status, *h_n_pairs, the first min(cap, n) pairs)"""
    dq, dqp, dt, dtp = ctx.to_device(q_surf), ctx.to_device(q_pose), ctx.to_device(t_surf), ctx.to_device(t_pose)
    d_pairs = ctx.alloc(8 * max(cap, 1))
    n = C.c_uint64(0)
    rc = ctx.lib.wc_match(ctx.h, C.c_void_p(dq.ptr), C.c_void_p(dqp.ptr), C.c_uint64(len(q_surf)), C.c_void_p(dt.ptr), C.c_void_p(dtp.ptr),
                          C.c_uint64(len(t_surf)), C.c_int(0), C.c_void_p(d_pairs.ptr), C.c_uint64(cap), C.byref(n), C.c_void_p(0), C.c_void_p(0))
    return rc, int(n.value), d_pairs.download(R.PAIR, min(cap, int(n.value)))


def test_failure_returns_and_the_call_after(oracle):
    """wc_match's own error codes, from finite inputs and one NaN (every index stays in range): a NaN centre in one target - WC_ERR_ARG;
    a fixed-window target stamped later than the query it is matched to - WC_ERR_ORDER; a pair capacity below the pair count -
    WC_ERR_CAPACITY with the full count in *h_n_pairs and the first `cap` pairs the reference's.  After each of them the next ordinary
    call on the same context returns the reference's pairs."""
    WC_ERR_CAPACITY, WC_ERR_ORDER, WC_ERR_ARG = 1, 3, 11
    w = synth.surfel_window(3, 120, seed=9, fixed_patches=90)
    q, qp, t, tp = w["surf"], w["pose"], w["fix_surf"], w["fix_pose"]
    P = M.params()
    ref = M.match(q, qp, t, tp, False, P)
    assert ref["rc"] == 0 and len(ref["pairs"]) > 40
    assert ref["pairs"].tobytes() == oracle.match(q, qp, t, tp, False).tobytes()
    ctx = lib.Context(0)
    try:
        def ordinary():
            assert ctx.match(q, qp, t, tp, False).tobytes() == ref["pairs"].tobytes()

        ordinary()
        bad = t.copy()
        bad["center"][17, 1] = np.nan
        rc, _, _ = _raw_match(ctx, q, qp, bad, tp, len(q))
        assert rc == WC_ERR_ARG, rc
        ordinary()
        late = t.copy()
        c0, q0 = int(ref["pairs"]["first"][5]), int(ref["pairs"]["second"][5])
        late["t"][c0] = q["t"][q0] + 1.0  # (the time gate still passes: this target stays q0's partner)
        assert M.match(q, qp, late, tp, False, P)["rc"] == WC_ERR_ORDER
        rc, _, _ = _raw_match(ctx, q, qp, late, tp, len(q))
        assert rc == WC_ERR_ORDER, rc
        ordinary()
        cap = len(ref["pairs"]) // 2
        few = M.match(q, qp, t, tp, False, P, cap=cap)
        assert few["rc"] == WC_ERR_CAPACITY and few["n_pairs"] == len(ref["pairs"]) and few["pairs"].tobytes() == ref["pairs"][:cap].tobytes()
        rc, n, pairs = _raw_match(ctx, q, qp, t, tp, cap)
        assert rc == WC_ERR_CAPACITY and n == len(ref["pairs"]), (rc, n)
        assert pairs.tobytes() == ref["pairs"][:cap].tobytes()
        ordinary()
    finally:
        ctx.close()
