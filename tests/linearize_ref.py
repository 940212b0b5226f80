"""H = J^T J, g = J^T r and the cost of a window, compared entry by entry in each entry's OWN scale, against a reference with short sums.

Metric.  H is positive semi-definite and c = 1/2 |r|^2 (for the loss-corrected residuals 1/2 r_c^2 <= 1/2 rho(r^2)), so by
Cauchy-Schwarz |H_ij| <= sqrt(H_ii H_jj) and |g_i| <= sqrt(H_ii) sqrt(2 c); the rounding error of any summation order of n terms
is at most gamma_n times those same bounds.  Hence
    eH = max_ij |H - H_ref|_ij / sqrt(H_ref_ii H_ref_jj),      eg = max_i |g - g_ref|_i / (sqrt(H_ref_ii) sqrt(2 c_ref))
over the rows with H_ref_ii > 0; a row whose reference diagonal is zero (the gauge rows, the bias rows of a window without IMU
factors) is a zero row of J and must be exactly zero on both sides.  The measure does not change when an unknown is rescaled - the
twelve unknowns of a sample state sit on scales nine decades apart, and a bar relative to max|H| sees the largest of them only.

Reference.  The oracle (oracle/window.cc) adds one factor after the other into its dense H in double.  The reference takes the
same oracle with SHORT sums: the binary and the unary pair lists cut into chunks, every chunk linearised in an oracle.Window of its
own (same sample times, gravity, gauge flag and parameters; loss and quirks act per factor, so chunking changes no term), one more
window with the IMU factors alone, and the chunk results added by Sum2 (Ogita, Rump and Oishi, SISC 2005: a running TwoSum, the
error terms collected in a second array) - as accurate as a sum in twice the working precision, in plain float64 on any machine
(no long double).  Chunk length 64, or what keeps a window at 512 chunks at most.

Bar of a device result: BAR_FACTOR * max(floor, FLOOR_MIN), the floor being the oracle's own sequential sums against this reference in
the same metric, computed per case (FLOOR_MIN: the largest floor measured at 8 to 127 sample states).  On top of it, only in the
sub-blocks they reach, come allowances for rounding noise of the REFERENCE's own factor evaluation, which no summation order removes.
Each is a stated multiple of what the oracle's evaluation was measured to be off by against mpmath (tests/test_linearize_ref.py
repeats those measurements and asserts the constants below), scaled by the case's inputs (allowances()); none comes from a device result.

 A. Jr.  The oracle forms Jr(r) with the coefficient (1 - cos th) / th (th = |r|): cos th is rounded next to 1, so the coefficient
    of hat(r / th) carries noise of the order u / th (u = 2^-53); measured: at most JR_NOISE u / th.  The device's 2 sin^2(th / 2) / th
    carries none, so this is one evaluation's noise.  Every Jacobian row with respect to a rotation is m^T Jr, so the rotation triple of
    a factor's row is off by at most JR_NOISE (u / th) |m|, |m| <= 1.1 |j| (Jr = I + O(th / 2), th <= 0.2).  Summed with Cauchy-Schwarz
    over the factors of a sample block I:
        |dH_ij| <= 1.1 JR_NOISE (u / th_min) sqrt(trace_rot H_II) sqrt(H_jj)   for i a rotation row of block I (twice if j is one too),
    in the metric 2 * 1.1 * sqrt(3) * JR_NOISE * (u / th_min) * kappa, kappa = the largest sqrt(max / min) of a block's three rotation
    diagonals, th_min = the smallest rotation correction any factor sees at x.  Zero at x = 0 (Jr = I).  Applied to rot x rot and rot x pos.
    In rot x b1 and rot x b2 the same noise is multiplied by |H_ij| / sqrt(H_ii H_jj) of those sub-blocks (2e-3 and below): under the
    plain bar, so they get nothing.
 B. The loss weight.  A surfel residual is w n . (R1 a1 + p1 - R2 a2 - p2): two lever arms of tens of metres rotated one by one, their
    difference millimetres, times a weight of up to 1 / sigma0.  In units of u w S, S = |a1| + |a2| + |p1| + |p2|, the oracle's residual
    was measured off by at most RES_NOISE (rms RES_RMS) over the unary factors of an 8-state window.  The device, which stores a1, a2
    and p1 - p2 per factor and sums in another order, is held to the same: two evaluations differ by at most
        dr = 2 * TAIL * RES_NOISE * u * w_max * S_max,     w_max = 1 / sigma0, S_max = 2 max|a| + 2 max|p|,
    TAIL = 4 because the sample is a hundred factors and a window holds up to two million, most of them with two corrected arms.
    The Cauchy corrector scales the factor's Jacobian row by sqrt(rho'(r^2)), rho' = 1 / (1 + r^2 / b), b = cauchy_a^2, and
    |d ln rho' / dr| = 2 r / (b + r^2) <= 1 / cauchy_a, so every term of the surfel factors' J^T J moves by up to dr / cauchy_a
    relative - in the metric, by Cauchy-Schwarz again, dr / cauchy_a.  Applied to pose x pose only (surfel factors have no other columns).
 Cost.  sum 1/2 rho(r^2) moves by sum rho' r dr_k.  The dr_k are roundings of different factors; added in quadrature, with
    rho'^2 r^2 <= rho' r^2 and sum rho' r^2 <= 2 c:  |dc| / c <= TAIL * sqrt(2) * RES_RMS * u * w_max * S_max * sqrt(2 / c).
 g keeps the plain bar.
 Residual classes: RES_FACTOR * eps of the class's largest value, plus: surfel residuals dr; gyroscope rows (a measured rate against
    Log of a product of three unit quaternions over dt: ~21 roundings of u per component in quadrature, the angle twice the vector
    part, two evaluations) GYR_NOISE u w_gyr / dt; accelerometer rows (R (acc - ba) + g, two vectors of 9.8 that cancel) ACC_NOISE u w_acc
    (max|acc| + |g|); bias rows nothing."""
import numpy as np

import lm_step_ref
from lm_step_ref import two_sum

TYPES = ("rot", "pos", "b1", "b2")  # local rows 0-2, 3-5, 6-8, 9-11 of a sample state
EPS = float(np.finfo(np.float64).eps)
FLOOR_MIN = 2.5e-15  # the largest floor measured (above): keeps a lucky case from setting a bar below rounding
BAR_FACTOR = 32.0    # tree instead of sequential sums (gamma_n, in the device's favour) and the fused SO(3) forms, a few ulp per call
RES_FACTOR = 64.0    # residual classes: RES_FACTOR * eps * max|class|
MAX_CHUNKS = 512
U = EPS / 2          # unit roundoff
JR_NOISE = 0.5       # the oracle's Jr against mpmath, in units of u / th: 0.42 at th = 3e-4, 0.24 at 1e-4, 0.07 at 1e-3 (200 directions each)
RES_NOISE = 0.6      # the oracle's surfel residual against mpmath, in units of u w S: largest of 100 unary factors 0.52 ...
RES_RMS = 0.2        # ... and their root mean square 0.17
TAIL = 4.0           # from a sample of a hundred factors to the largest of a window's
GYR_NOISE = 8.0      # 2 * sqrt(21 / 3) u per evaluation, two evaluations in quadrature: 7.5
ACC_NOISE = 2.0


# ---- the window as plain data ------------------------------------------------------------------------------------------------------
def spec(w, params, pairs, pf, fix_first, imu):
    """what defines a window problem: w (synth.surfel_window), the binary and unary pair lists, the gauge flag, the IMU states or None"""
    return dict(w=w, params=params, pairs=pairs, pf=pf, fix_first=bool(fix_first), imu=imu)


def from_problem(prob):
    """the spec of an lm_step_ref.window_problem"""
    return spec(prob["w"], prob["params"], prob["pairs"], prob["pf"], prob["fix_first"], prob["imu"])


def _window(oracle, sp, pairs, pf, imu):
    w = sp["w"]
    W = oracle.Window(w["sample_times"], w["grav"], sp["fix_first"], sp["params"])
    if pairs is not None and len(pairs):
        W.add_binary(w["surf"], w["pose"], pairs)
    if pf is not None and len(pf):
        W.add_unary(w["fix_surf"], w["fix_pose"], w["surf"], w["pose"], pf)
    if imu is not None:
        W.add_imu(imu)
    return W


def oracle_window(oracle, sp):
    """the whole problem in one oracle.Window (insertion order of the reference: binary, unary, IMU)"""
    return _window(oracle, sp, sp["pairs"], sp["pf"], sp["imu"])


# ---- Sum2 ------------------------------------------------------------------------------------------------------------------------------
class Sum2:
    """running sum of arrays of one shape: s by TwoSum, the error terms in e; value() = s + e"""

    def __init__(self, shape):
        self.s, self.e = np.zeros(shape), np.zeros(shape)

    def add(self, a, idx=None):
        """+= a; idx (np.ix_ or an index array): a holds the entries at idx only"""
        if idx is None:
            self.s, q = two_sum(self.s, a)
            self.e += q
        else:
            s, q = two_sum(self.s[idx], a)
            self.s[idx] = s
            self.e[idx] += q

    def value(self):
        return self.s + self.e


def chunk_length(n_factors, chunk=64):
    return max(chunk, -(-n_factors // MAX_CHUNKS))


def reference(oracle, sp, x, chunk=None):
    """(H, g, cost) at x from chunk linearisations added by Sum2; chunk: factors per chunk (default: chunk_length)"""
    ns = len(sp["w"]["sample_times"])
    n = 12 * ns
    x = np.ascontiguousarray(x, np.float64)
    chunk = chunk or chunk_length(len(sp["pairs"]) + len(sp["pf"]))
    aH, ag, ac = Sum2((n, n)), Sum2(n), Sum2(())

    def add(W):
        H, g, c = W.linearize(x)
        rows = np.nonzero(np.diag(H))[0]  # a zero diagonal entry of J^T J is a zero column of J: nothing else in that row
        if 2 * len(rows) < n:
            aH.add(H[np.ix_(rows, rows)], np.ix_(rows, rows))
            ag.add(g[rows], rows)
        else:
            aH.add(H)
            ag.add(g)
        ac.add(c)

    for k in range(0, len(sp["pairs"]), chunk):
        add(_window(oracle, sp, sp["pairs"][k:k + chunk], None, None))
    for k in range(0, len(sp["pf"]), chunk):
        add(_window(oracle, sp, None, sp["pf"][k:k + chunk], None))
    if sp["imu"] is not None:
        add(_window(oracle, sp, None, None, sp["imu"]))
    return aH.value(), ag.value(), float(ac.value())


# ---- the comparison ------------------------------------------------------------------------------------------------------------------
def _where(i, j=None):
    if j is None:
        return "block %d local row %d (%s)" % (i // 12, i % 12, TYPES[i % 12 // 3])
    return "block pair (%d, %d) local (%d, %d) sub-block %s x %s" % (i // 12, j // 12, i % 12, j % 12, TYPES[i % 12 // 3], TYPES[j % 12 // 3])


def scaled_errors(H, g, cost, H_ref, g_ref, cost_ref):
    """dict: eH, eg, ec (relative cost difference); eH_types (4 x 4) and eg_types (4): the same maxima by unknown type; dead_exact: the
    rows with a zero reference diagonal are exactly zero in H, g, H_ref and g_ref; where_H / where_g: the arg-max spelled out"""
    n = len(g_ref)
    ns = n // 12
    d = np.sqrt(np.diag(H_ref))
    dead = ~(d > 0)
    inv = np.where(dead, 0.0, 1.0 / np.where(dead, 1.0, d))
    E = np.abs(H - H_ref)
    E *= inv[:, None]
    E *= inv[None, :]
    eg_all = np.abs(g - g_ref) * inv / np.sqrt(2.0 * cost_ref)
    dead_exact = not (H[dead].any() or H[:, dead].any() or H_ref[dead].any() or H_ref[:, dead].any() or g[dead].any() or g_ref[dead].any())
    i, j = np.unravel_index(int(np.argmax(E)), E.shape)
    k = int(np.argmax(eg_all))
    out = dict(eH=float(E[i, j]), eg=float(eg_all[k]), ec=abs(cost - cost_ref) / cost_ref, dead_exact=dead_exact, n_dead=int(dead.sum()),
               eH_types=E.reshape(ns, 4, 3, ns, 4, 3).max(axis=(0, 2, 3, 5)), eg_types=eg_all.reshape(ns, 4, 3).max(axis=(0, 2)),
               where_H="%s: %.17g against %.17g" % (_where(i, j), H[i, j], H_ref[i, j]),
               where_g="%s: %.17g against %.17g" % (_where(k), g[k], g_ref[k]))
    return out


def describe(e):
    """one line per number: the failure message of a case"""
    lines = ["eH %.2e at %s" % (e["eH"], e["where_H"]), "eg %.2e at %s" % (e["eg"], e["where_g"]), "cost %.2e" % e["ec"], "eH by type (rows / columns %s):" % " ".join(TYPES)]
    lines += ["  %-3s " % TYPES[a] + " ".join("%.1e" % v for v in e["eH_types"][a]) for a in range(4)]
    lines.append("eg by type: " + " ".join("%s %.1e" % (TYPES[a], e["eg_types"][a]) for a in range(4)))
    return "\n".join(lines)


def _corrections(times, X, t):
    """|rotation correction| interpolated at the stamps t between the bracketing sample states"""
    l = np.clip(np.searchsorted(times, t, side="right") - 1, 0, len(times) - 2)
    f = ((t - times[l]) / (times[l + 1] - times[l]))[:, None]
    return np.linalg.norm((1 - f) * X[l, 0:3] + f * X[l + 1, 0:3], axis=1)


def allowances(sp, x, H_ref, c_ref):
    """the reference's own evaluation noise at x, derived from the inputs (module docstring): dict jr (A, in the metric), loss (B, in the
    metric), cost (B's share of the relative cost difference) and the residual classes' absolute allowances surfel, gyr, acc"""
    w, P = sp["w"], sp["params"]
    times = np.asarray(w["sample_times"], np.float64)
    ns = len(times)
    X = np.asarray(x, np.float64).reshape(ns, 12)
    th = [np.zeros(0)]
    used = np.unique(np.concatenate([sp["pairs"]["first"], sp["pairs"]["second"], sp["pf"]["second"]]))
    if len(used):
        th.append(_corrections(times, X, w["surf"]["t"][used]))
    imu = sp["imu"]
    if imu is not None:
        th.append(_corrections(times, X, imu["t"][(imu["t"] >= times[0]) & (imu["t"] <= times[-1])]))
    th = np.concatenate(th)
    th = th[th > 0]
    d = np.diag(H_ref).reshape(ns, 4, 3)[:, 0, :]
    live = d.min(axis=1) > 0
    kappa = float(np.sqrt((d[live].max(axis=1) / d[live].min(axis=1)).max())) if live.any() else 1.0
    jr = 2 * 1.1 * np.sqrt(3.0) * JR_NOISE * (U / th.min()) * kappa if len(th) else 0.0
    out = dict(jr=float(jr), loss=0.0, cost=0.0, surfel=0.0, gyr=0.0, acc=0.0, th_min=float(th.min()) if len(th) else 0.0, kappa=kappa)
    if len(used):
        arm = max(np.linalg.norm(w["surf"]["center"], axis=1).max(), np.linalg.norm(w["fix_surf"]["center"], axis=1).max() if len(sp["pf"]) else 0.0)
        pos = max(np.linalg.norm(w["pose"]["pos"], axis=1).max(), np.linalg.norm(w["fix_pose"]["pos"], axis=1).max() if len(sp["pf"]) else 0.0)
        unit = U / P.surfel_sigma0 * 2 * (arm + pos)  # u w_max S_max
        out["surfel"] = float(2 * TAIL * RES_NOISE * unit)
        out["loss"] = out["surfel"] / P.cauchy_a
        out["cost"] = float(TAIL * np.sqrt(2.0) * RES_RMS * unit * np.sqrt(2.0 / c_ref))
    if imu is not None:
        out["gyr"] = float(GYR_NOISE * U * P.w_gyr / P.imu_dt)
        out["acc"] = float(ACC_NOISE * U * P.w_acc * (np.linalg.norm(imu["acc"], axis=1).max() + np.linalg.norm(w["grav"])))
    return out


def bars(floor, allow=None):
    """(4 x 4 bars of eH by unknown-type pair, bar of eg and of every type, bar of the cost) from a case's CPU floor (the oracle's
    sequential sums against the reference, scaled_errors of it) and, for a device result, the reference's evaluation noise (allowances):
    B in pose x pose, A in rot x rot and rot x pos, the cost's share; every pair with a bias row or column keeps the plain bar"""
    bH = np.full((4, 4), BAR_FACTOR * max(floor["eH"], FLOOR_MIN))
    if allow:
        bH[:2, :2] += allow["loss"]
        bH[0, :2] += allow["jr"]
        bH[1, 0] += allow["jr"]
    return bH, BAR_FACTOR * max(floor["eg"], FLOOR_MIN), BAR_FACTOR * max(floor["ec"], EPS) + (allow["cost"] if allow else 0.0)


def within(e, floor, allow=None):
    """assertions 1 and 2: every type pair of eH (so eH itself), eg and every type of it, and the cost below the bar"""
    bH, bg, bc = bars(floor, allow)
    return bool(np.all(e["eH_types"] <= bH) and e["eg"] <= bg and e["ec"] <= bc and np.all(e["eg_types"] <= bg))


def subblock_nonzero(H):
    """(ns, 4, ns, 4) bool: which 3 x 3 sub-blocks (by unknown type, inside every 12 x 12 block) hold a non-zero entry"""
    ns = len(H) // 12
    return np.abs(H).reshape(ns, 4, 3, ns, 4, 3).max(axis=(2, 5)) != 0


def residual_errors(res, res_ref, n_surfel):
    """per residual class (surfel residuals; each of the 12 components of the IMU residual over all IMU factors):
    [(name, max|difference|, max|reference|)]; a residual vector is n_surfel surfel residuals, then 12 per IMU factor"""
    out = [("surfel", float(np.abs(res[:n_surfel] - res_ref[:n_surfel]).max()) if n_surfel else 0.0,
            float(np.abs(res_ref[:n_surfel]).max()) if n_surfel else 0.0)]
    a, b = res[n_surfel:].reshape(-1, 12), res_ref[n_surfel:].reshape(-1, 12)
    if len(b):
        out += [("imu[%d]" % k, float(np.abs(a[:, k] - b[:, k]).max()), float(np.abs(b[:, k]).max())) for k in range(12)]
    return out


def residual_bar(name, scale, allow=None):
    """RES_FACTOR * eps of the class's largest reference value, plus the class's own cancellation (allowances); an all-zero class: 0"""
    if scale == 0:
        return 0.0
    extra = 0.0
    if allow:
        extra = allow["surfel"] if name == "surfel" else allow["gyr"] if name in ("imu[0]", "imu[1]", "imu[2]") else allow["acc"] if name in ("imu[3]", "imu[4]", "imu[5]") else 0.0
    return RES_FACTOR * EPS * scale + extra


def residuals_within(classes, allow=None):
    return all(err <= residual_bar(name, scale, allow) for name, err, scale in classes)


# ---- the bars the suite had before (tests/test_window_gpu.py), kept to show what they let through ---------------------------------------
def old_bars(H, g, cost, H_ref, g_ref, cost_ref):
    """dict of bool: 'small' (test_evaluate_and_linearize_match_oracle: 1e-10 of max|H| / max|g|, cost 1e-11), 'large' (the C3 / C4 /
    large-window tests: 1e-9, every 12 x 12 block to 1e-8 of its own maximum + 1e-12 max|H|, the same block sparsity, cost 1e-10),
    'golden' (test_golden.py: 2e-6 max|H|)"""
    ns = len(g_ref) // 12
    dH, dg = np.abs(H - H_ref).max(), np.abs(g - g_ref).max()
    mH, mg = np.abs(H_ref).max(), np.abs(g_ref).max()
    Hb = np.abs(H - H_ref).reshape(ns, 12, ns, 12).max(axis=(1, 3))
    Hs = np.abs(H_ref).reshape(ns, 12, ns, 12).max(axis=(1, 3))
    blocks = np.all(Hb <= 1e-8 * np.maximum(Hs, 1e-300) + 1e-12 * mH) and np.array_equal(Hs == 0, np.abs(H).reshape(ns, 12, ns, 12).max(axis=(1, 3)) == 0)
    sym = np.array_equal(H, H.T)
    return dict(small=bool(sym and dH <= 1e-10 * mH and dg <= 1e-10 * mg and abs(cost - cost_ref) <= 1e-11 * cost_ref),
                large=bool(sym and dH <= 1e-9 * mH and dg <= 1e-9 * mg and blocks and abs(cost - cost_ref) <= 1e-10 * cost_ref),
                golden=bool(dH <= 2e-6 * mH))


# ---- a device result against the reference: the assertions of tests/test_linearize_gpu.py ------------------------------------------------
def random_point(ns, seed):
    return 2e-3 * np.random.default_rng(seed).normal(size=12 * ns)


def check_linearization(oracle, sp, results, tag, W=None, log=None):
    """results: one dict per point, computed elsewhere (a device): x, H, g, cost, and optionally eval_cost and res (cost and residual
    vector of an evaluation at x) and oracle (W.linearize(x), if the caller has it); x = 0 first, a random point last.  log: a list that
    receives (where, ns, floor, errors or residual classes, allowances, bars) per point.  Asserts per point: eH, eg, cost and every unknown-type pair below
    the bar set from the CPU floor of this case; exact symmetry; exact zeros in the rows whose reference diagonal is zero; the entry
    sparsity of the reference at 3 x 3 sub-block granularity (the structure is the reference's at the random point, where no entry
    is zero by value only; at x = 0 nothing outside that structure may be written and nothing of the reference may be missing);
    residuals by class.  W: the whole problem's oracle.Window if the caller has it already.  Returns [(floor, device errors)]."""
    W = W or oracle_window(oracle, sp)
    ns = W.ns
    out = []
    structure = None
    for r in reversed(results):  # (the random point first: it defines the structure)
        x, H, g = r["x"], r["H"], r["g"]
        H_ref, g_ref, c_ref = reference(oracle, sp, x)
        floor = scaled_errors(*(r.get("oracle") or W.linearize(x)), H_ref, g_ref, c_ref)
        e = scaled_errors(H, g, r["cost"], H_ref, g_ref, c_ref)
        allow = allowances(sp, x, H_ref, c_ref)
        bH, bg, bc = bars(floor, allow)
        at = "%s at %s" % (tag, "x = 0" if not np.any(x) else "the random point")
        if log is not None:
            log.append((at, ns, floor, e, allow, (bH, bg, bc)))
        assert floor["dead_exact"], (at, "the oracle against its own short sums", describe(floor))
        assert within(e, floor, allow), "%s: above the bar (eg %.2e, cost %.2e, eH by type:\n%s)\n%s" % (at, bg, bc, np.array2string(bH, precision=1), describe(e))
        assert np.array_equal(H, H.T), at
        assert e["dead_exact"], (at, "rows with a zero reference diagonal are not exactly zero")
        if sp["fix_first"]:
            assert not H[3:6].any() and not H[:, 3:6].any() and not g[3:6].any(), at
        nz, nz_ref = subblock_nonzero(H), subblock_nonzero(H_ref)
        if structure is None:
            assert np.any(x), "the last point must be a random one"
            structure = nz_ref
            diff = np.argwhere(nz != nz_ref)
            assert len(diff) == 0, (at, "3 x 3 sub-block sparsity differs", [(int(a), TYPES[b], int(c), TYPES[d_]) for a, b, c, d_ in diff[:8]])
        else:
            assert not np.any(nz & ~structure), (at, "a structurally zero sub-block was written", np.argwhere(nz & ~structure)[:8].tolist())
            assert not np.any(nz_ref & ~nz), (at, "a sub-block of the reference is missing", np.argwhere(nz_ref & ~nz)[:8].tolist())
        if r.get("eval_cost") is not None:
            assert abs(r["eval_cost"] - c_ref) <= bc * c_ref, (at, "cost of the evaluation", r["eval_cost"], c_ref)
        if r.get("res") is not None:
            _, res_ref = W.evaluate(x, want_residuals=True)
            assert len(r["res"]) == len(res_ref), at
            classes = residual_errors(r["res"], res_ref, len(res_ref) - 12 * (W.counts()[4] + W.counts()[5]))
            if log is not None:
                log.append((at + " residuals", ns, None, classes, allow, None))
            assert residuals_within(classes, allow), (at, "residual classes", [c + (residual_bar(c[0], c[2], allow),) for c in classes if c[1] > residual_bar(c[0], c[2], allow)])
        out.append((floor, e))
    return out[::-1]


# windows of tests/lm_step_ref.py, re-exported for the two test files
FAMILIES = lm_step_ref.FAMILIES
window_problem = lm_step_ref.window_problem
window_shape = lm_step_ref.window_shape
