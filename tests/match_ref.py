"""The surfel matcher in plain numpy - TEST INFRASTRUCTURE.

A brute-force float64 restatement of KnnSurfelMatcher::Match as oracle/match.cc states it, operation for operation:

  features   world centre and normal through qrot in oracle/math3.h's order (uv = u x v; uv += uv; v + w uv + u x uv), the centre plus
             the pose's position, divided by center_scale / angular_scale
  distances  flann::L2_Simple: a plain left-to-right sum of the six squared differences
  lists      the k smallest by (distance, index); fewer than k targets: the tail stays (index 0, distance 0) (Q10)
  gates      cc:26 fabs(dt) < time_diff_min, cc:29 acos(dot(nq, nc)) > angular_scale (math.acos: the libm the oracle calls; a dot product
             outside [-1, 1] is NaN there and NaN passes), cc:32 fabs(dot(nq, cq - ct)) > surfel_dist_max
  pairing    the std::set rule in query order (cc:35-38), a pair as (older, newer); two sets: (target, query), the target must be older

No kd-tree: O(nq nt), meant for a few thousand surfels.  Neither the oracle's arithmetic nor the device's is contracted into fused
multiply-adds (-ffp-contract=off on both), so every operand below is the one they compare.

match() also returns, per query and list entry, the three gate operands and which gates passed: tests/match_gates.py builds its cases on
them and the tests assert on them.  early_operands() restates what the EARLY walk of csrc/match_tree.inc accepts a candidate on (computed
from the features, not from the gates' operands): the scenes are checked to reach into its margins with it.  Nothing here runs on a GPU."""
import math
from types import SimpleNamespace

import numpy as np

from wildcat_slam_amd import records as R


def params(**over):
    """what the matcher reads of a wc_params: the reference's values, and overrides"""
    p = SimpleNamespace(knn_k=10, center_scale=1.0, angular_scale=5.0 * math.pi / 180.0, surfel_dist_max=0.1, time_diff_min=0.06)
    for k_, v in over.items():
        setattr(p, k_, v)
    return p


def to_wc_params(p, base):
    """`base` (a wc_params with the defaults) with the matcher's five fields taken from p"""
    for f in ("knn_k", "center_scale", "angular_scale", "surfel_dist_max", "time_diff_min"):
        setattr(base, f, getattr(p, f))
    return base


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def qrot(q, v):
    """math3.h:116-121, quaternion (w, x, y, z)"""
    u, w = q[:, 1:4], q[:, 0:1]
    uv = _cross(u, v)
    uv = uv + uv
    return (v + w * uv) + _cross(u, uv)


def world(surf, pose):
    """(centre, normal) in the world frame: GetCenterInWorld / GetNormInWorld"""
    q = np.ascontiguousarray(pose["quat"], np.float64)
    return qrot(q, np.ascontiguousarray(surf["center"], np.float64)) + pose["pos"], qrot(q, np.ascontiguousarray(surf["normal"], np.float64))


def features(surf, pose, P):
    cw, nw = world(surf, pose)
    return np.concatenate([cw / P.center_scale, nw / P.angular_scale], 1)


def dist2(fq, ft):
    """squared distances of one query feature to every target, L2_Simple's order"""
    s = np.zeros(len(ft))
    for d in range(6):
        df = fq[d] - ft[:, d]
        s = s + df * df
    return s


def knn(ft, fq, k):
    """-> (idx int32 [nq, k], d2 [nq, k]) as wco_knn6 returns them"""
    nq, nt = len(fq), len(ft)
    idx, d2 = np.zeros((nq, k), np.int32), np.zeros((nq, k))
    ids = np.arange(nt)
    for q in range(nq):
        s = dist2(fq[q], ft)
        if nt > 4 * k:  # (only the candidates up to the k-th smallest distance need the full order)
            kth = np.partition(s, k - 1)[k - 1]
            cand = ids[s <= kth]
        else:
            cand = ids
        o = cand[np.lexsort((cand, s[cand]))][:k]
        idx[q, : len(o)], d2[q, : len(o)] = o, s[o]
    return idx, d2


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _acos(x):
    try:
        return math.acos(x)
    except ValueError:  # outside [-1, 1] (or NaN): std::acos returns NaN
        return math.nan


def gate_operands(tq, cq, nq, tc, cc, nc):
    """the three operands of cc:26 / cc:29 / cc:32 for one (query, candidate): (fabs(dt), dot, acos(dot), fabs(plane))"""
    dt = abs(float(tc) - float(tq))
    d = float(_dot(nq, nc))
    return dt, d, _acos(d), abs(float(_dot(nq, cq - cc)))


def gates_pass(ops, P):
    dt, _, ang, pl = ops
    return (not dt < P.time_diff_min), (not ang > P.angular_scale), (not pl > P.surfel_dist_max)


def match(q_surf, q_pose, t_surf, t_pose, same_set, P, cap=None, lists=None):
    """-> dict(rc (0, 1 capacity, 3 order: wco_match's), n_pairs (the full count), pairs [PAIR, at most cap], idx, d2 (the lists),
    dt, dot, ang, plane [nq, k] (the gates' operands per list entry), passed [nq, k, 3] (time, angle, plane), chosen [nq] (the
    candidate a query was paired with, -1: none)).  lists: (idx, d2) of a call with a larger k on the same sets (a prefix is the list)"""
    nq, nt, k = len(q_surf), len(t_surf), int(P.knn_k)
    cap = nq if cap is None else cap
    out = dict(rc=0, n_pairs=0, pairs=np.zeros(0, R.PAIR), idx=np.zeros((nq, k), np.int32), d2=np.zeros((nq, k)), dt=np.zeros((nq, k)),
               dot=np.zeros((nq, k)), ang=np.zeros((nq, k)), plane=np.zeros((nq, k)), passed=np.zeros((nq, k, 3), bool), chosen=np.full(nq, -1, np.int64))
    if nt == 0:
        return out
    tcw, tnw = world(t_surf, t_pose)
    qcw, qnw = (tcw, tnw) if same_set else world(q_surf, q_pose)
    if lists is None:
        ft = np.concatenate([tcw / P.center_scale, tnw / P.angular_scale], 1)
        fq = ft if same_set else np.concatenate([qcw / P.center_scale, qnw / P.angular_scale], 1)
        idx, d2 = knn(ft, fq, k)
    else:
        idx, d2 = lists[0][:, :k].copy(), lists[1][:, :k].copy()
        if nt < k:
            idx[:, nt:], d2[:, nt:] = 0, 0.0
    out["idx"], out["d2"] = idx, d2
    tt, tq_ = t_surf["t"], q_surf["t"]
    seen = set()
    pairs = []
    n = 0
    for q in range(nq):
        qid = q if same_set else -q - 1
        took = False
        for j in range(k):
            c = int(idx[q, j])
            ops = gate_operands(tq_[q], qcw[q], qnw[q], tt[c], tcw[c], tnw[c])
            ps = gates_pass(ops, P)
            out["dt"][q, j], out["dot"][q, j], out["ang"][q, j], out["plane"][q, j] = ops
            out["passed"][q, j] = ps
            if took or not all(ps):
                continue
            if (qid, c) in seen or (c, qid) in seen:
                continue
            seen.add((qid, c))
            if n < cap:
                if same_set:
                    pairs.append((q, c) if tq_[q] < tt[c] else (c, q))
                else:
                    if not tt[c] < tq_[q]:
                        out["rc"] = 3
                        out["pairs"] = np.array(pairs, R.PAIR) if pairs else np.zeros(0, R.PAIR)
                        return out
                    pairs.append((c, q))
            n += 1
            out["chosen"][q] = c
            took = True  # (the reference breaks here; the remaining entries only get their operands recorded)
    out["n_pairs"] = n
    out["pairs"] = np.array(pairs, R.PAIR) if pairs else np.zeros(0, R.PAIR)
    out["rc"] = 1 if n > cap else 0
    return out


def early_operands(fq, ft, P):
    """what the EARLY walk accepts candidate features ft [m, 6] of query feature fq on (match_tree.inc, the leaf loop):
    -> (cosine = dn as as, plane = fabs(dp) as cs, qmax), dn and dp summed in the loop's order"""
    a, c = P.angular_scale, P.center_scale
    dn, dp = np.zeros(len(ft)), np.zeros(len(ft))
    for d in range(6):
        pv = ft[:, d]
        df = fq[d] - pv
        if d >= 3:
            dn = dn + fq[d] * pv
        else:
            dp = dp + fq[d + 3] * df
    return dn * a * a, np.abs(dp) * a * c, float(np.max(np.abs(fq)))


def early_margins(P):
    """(cos_acc, plane_acc) as match_impl sets them (csrc/match.hip)"""
    a = P.angular_scale
    cos_acc = math.cos(min(a, 3.141592653589793) - 1e-9) + 1e-12 if a > 1e-8 else 2.0
    return cos_acc, P.surfel_dist_max * (1.0 - 1e-9) - 1e-12
