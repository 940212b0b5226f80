"""The decisions of the window solver's LM loop (csrc/lm_loop.h) without a GPU, through the header's g++ instantiation in the facade
library (host/odom_c_api.cc: wc_host_lm_loop) - the same header wc_window_solve (csrc/window.hip) drives on the device.

1. Against the independent numpy loop (tests/lm_loop_ref.py), on every scenario of lm_loop_ref.SCENARIOS: a second driver with the same
   linearize / evaluate callbacks and the same lm_step_ref step, every decision taken by the header.  Both drivers feed identical
   doubles, so the comparison is equality: trajectory, every record's radius, the counts, termination, final cost and best x, under
   every max_iterations = k prefix (k = 0 included; on ALL scenarios - the callbacks' results are kept per point, so the sweep costs
   little), dense re-tries = lm_loop_ref.expected_retries.
2. Scripted mails: each decision at its threshold, the run of rejections down to radius <= 1e-32 (which no window reaches), the
   radius cap, the lm_dense_radius switch, the dense re-try, lm_radius0.  Every script also runs through `expected`, the decisions
   restated in Python, which must agree attempt by attempt.
3. The late gradient of the two-collective form: every script in both forms, the summaries equal field by field, the attempts equal
   but for the one more attempt the late form asks for when an accepted point's gradient is at or below the tolerance.
4. `expected(fault=...)` with three single mistakes: each is caught by at least one script."""
import ctypes as C
import math
import os
from collections import namedtuple

import numpy as np
import pytest

import lm_loop_ref as ref
import lm_step_ref as step_ref
from wildcat_slam_amd import lib

STOP, ELIMINATION, DENSE = 0, 1, 2                      # LmAction
STOPPED, RETRY, INVALID, ACCEPTED, REJECTED = range(5)  # LmVerdict
VERDICT = {STOPPED: "S", RETRY: "R", INVALID: "x", ACCEPTED: "+", REJECTED: "-"}
OUT = ("cost", "gmax", "min_cost", "radius", "decrease", "x_norm", "iter", "consecutive_invalid", "first_recorded", "first_step_now",
       "late_pending", "late_at", "initial_cost", "final_cost", "iterations", "successful_steps", "unsuccessful_steps", "termination",
       "n_linearizations", "n_cost_evaluations", "first_step0", "retries")
SUMMARY = OUT[12:]
INF, NAN = math.inf, math.nan


def up(v):
    return math.nextafter(v, INF)


@pytest.fixture(scope="module")
def host():
    lib.load()
    so = os.path.join(os.path.dirname(lib.so_path()), "..", "host", "libwildcat_odometry.so")
    h = C.CDLL(os.path.abspath(so))
    assert hasattr(h, "wc_host_lm_loop")
    h.wc_host_lm_loop.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    return h


class Loop:
    """a caller-owned LmLoop block and the header's four calls; self[...] = the state after the last call"""

    def __init__(self, host, cost, gmax, x_norm, max_iterations=50, radius0=-1, dense_radius=7, dense=0, ns=14, late=0):
        self.host = host
        self.block = C.create_string_buffer(host.wc_host_lm_loop(-1, None, 0, None, None))
        self._call(0, max_iterations, radius0, dense_radius, dense, ns, late, cost, gmax, x_norm)

    def _call(self, op, *args):
        a, out = (C.c_double * max(len(args), 1))(*args), (C.c_double * len(OUT))()
        rc = self.host.wc_host_lm_loop(op, self.block, len(self.block), a, out)
        assert rc >= 0, (op, rc)
        self.state = dict(zip(OUT, out))
        return rc

    def next(self):
        return self._call(1)

    def judge(self, fail, model_change, step_norm, cand_cost, cand_gmax, late_gmax=0.0):
        return self._call(2, fail, model_change, step_norm, cand_cost, cand_gmax, late_gmax)

    def accepted(self, x_norm, slot=0):
        return bool(self._call(3, x_norm, slot))

    def __getitem__(self, f):
        return self.state[f]

    def summary(self):
        return {f: self.state[f] for f in SUMMARY}


def test_the_block_is_checked(host):
    size = host.wc_host_lm_loop(-1, None, 0, None, None)
    assert 0 < size <= 512
    buf, a = C.create_string_buffer(size), (C.c_double * 9)()
    assert host.wc_host_lm_loop(0, buf, size - 1, a, None) == -2 and host.wc_host_lm_loop(0, None, size, a, None) == -2
    assert host.wc_host_lm_loop(7, buf, size, a, None) == -2 and host.wc_host_lm_loop(2, buf, size, None, None) == -2


# ---- 1. the scenarios ----------------------------------------------------------------------------------------------------------
class Callbacks:
    """a scenario's linearize / evaluate / step, each result kept per argument: the prefixes ask for the same ones again"""

    def __init__(self, W):
        self.W, self.lin, self.ev, self.st = W, {}, {}, {}

    def linearize(self, x):
        k = x.tobytes()
        if k not in self.lin:
            self.lin[k] = self.W.linearize(x)
        return self.lin[k]

    def evaluate(self, x):
        k = x.tobytes()
        if k not in self.ev:
            self.ev[k] = self.W.evaluate(x)
        return self.ev[k]

    def step(self, x, H, g, radius, scale, refine=3):
        """lm_loop's step, formed as lm_loop forms it -> (ok, y, model_change)"""
        k = (x.tobytes(), radius)
        if k not in self.st:
            A, gs, _ = step_ref.damped_system(H, g, radius, scale)
            Hs = H * scale[:, None] * scale[None, :]
            try:
                with np.errstate(all="ignore"):
                    y = step_ref.solve(A, gs, refine)
                model_change = float(y @ gs - 0.5 * (y @ (Hs @ y)))
                self.st[k] = (bool(np.all(np.isfinite(y))) and model_change > 0, y, model_change)
            except np.linalg.LinAlgError:
                self.st[k] = (False, None, NAN)
        return self.st[k]


_CALLBACKS = {}


def callbacks(oracle, name):
    if name not in _CALLBACKS:
        _CALLBACKS[name] = Callbacks(step_ref.oracle_window(oracle, ref.reference(oracle, name)[0]))
    return _CALLBACKS[name]


def header_loop(host, cb, prob, max_iterations, dense=0):
    """lm_loop_ref.lm_loop with every decision taken by the header -> (trace, summary, dense re-tries).  As on the device, the
    candidate's linearisation belongs to the attempt: its max |g| is in the mail that is judged"""
    x = np.array(prob["x0"], np.float64)
    H, g, cost = cb.linearize(x)
    scale = 1.0 / (1.0 + np.sqrt(np.diag(H)))
    best = x.copy()
    L = Loop(host, cost, np.abs(g).max(), np.linalg.norm(x), max_iterations, int(round(np.log10(prob["radius0"]))), 7, dense, prob["ns"])
    trace = []
    while True:
        act = L.next()
        if act == STOP:
            break
        radius, x_norm = L["radius"], L["x_norm"]
        ok, y, model_change = cb.step(x, H, g, radius, scale)
        if ok:
            cand = x - scale * y
            mail = (0, model_change, float(np.linalg.norm(x - cand)), cb.evaluate(cand), np.abs(cb.linearize(cand)[1]).max())
        else:
            mail = (1, model_change, NAN, NAN, NAN)
        v = L.judge(*mail)
        if v == RETRY:  # (the numpy loop has one step form: the dense re-try finds the same step)
            assert act == ELIMINATION and radius <= ref.SWITCH
            v = L.judge(*mail)
        assert v != RETRY
        step_ratio = mail[2] / (1e-8 * (x_norm + 1e-8)) if ok else None
        cost_ratio = float(abs(cost - mail[3]) / (1e-6 * cost)) if ok else None
        rho = (cost - mail[3]) / model_change if ok else None
        if v == ACCEPTED:
            x = cand
            H, g, cost = cb.linearize(x)
            assert cost == mail[3]  # (the oracle's two passes give one cost: both drivers go on from the same doubles)
            if L.accepted(np.linalg.norm(x)):
                best = x.copy()
            kind = ref.ACCEPTED
        elif v == STOPPED and ok:  # on a tolerance: the parameter tolerance is tested first
            kind = ref.PARAMETER_TOLERANCE if step_ratio <= 1.0 else ref.FUNCTION_TOLERANCE
        else:
            kind = {REJECTED: ref.REJECTED, INVALID: ref.INVALID, STOPPED: ref.INVALID}[v]
        trace.append(ref.Record(kind, radius, rho if kind in (ref.ACCEPTED, ref.REJECTED) else None, step_ratio,
                                cost_ratio if kind != ref.PARAMETER_TOLERANCE else None, L["min_cost"], best.copy()))
    s = L.summary()
    return trace, ref.Summary(int(s["iterations"]), int(s["successful_steps"]), int(s["unsuccessful_steps"]), int(s["termination"]),
                              int(s["n_linearizations"]), s["initial_cost"], s["final_cost"], best.copy()), s["retries"]


def same_summary(a, b):
    return a[:7] == b[:7] and a.x.tobytes() == b.x.tobytes()


@pytest.mark.parametrize("name", tuple(ref.SCENARIOS))
def test_header_takes_the_numpy_loops_decisions(host, oracle, name):
    prob, trace, want = ref.reference(oracle, name)
    cb = callbacks(oracle, name)
    for form, dense in (("default", 0), ("dense", 1)):
        got_trace, got, retries = header_loop(host, cb, prob, prob["params"].max_iterations, dense)
        assert ref.trajectory(got_trace) == ref.trajectory(trace), (name, form)
        assert [r.radius for r in got_trace] == [r.radius for r in trace], (name, form)  # (floats compared with ==: bit for bit, no NaN here)
        for a, b in zip(got_trace, trace):
            assert a[:6] == b[:6] and a.x.tobytes() == b.x.tobytes(), (name, form, a[:6], b[:6])
        assert same_summary(got, want), (name, form, got[:7], want[:7])
        assert retries == ref.expected_retries(prob, trace, form), (name, form, retries)


@pytest.mark.parametrize("name", tuple(ref.SCENARIOS))
def test_header_prefixes(host, oracle, name):
    """max_iterations = k for every k from 0 to one past the trace's end: the trace's first k records, its counts, termination 1
    while cut short, the best point and cost after k iterations, the re-tries of the first k iterations"""
    prob, trace, want = ref.reference(oracle, name)
    cb = callbacks(oracle, name)
    for form, dense in (("default", 0), ("dense", 1)):
        for k in range(0, want.iterations + 2):
            got_trace, got, retries = header_loop(host, cb, prob, k, dense)
            if k < want.iterations:
                it, good, bad, cost, x_k = ref.prefix(trace, k, prob["x0"], want.initial_cost)
                assert got[:5] == (it, good, bad, 1, 1 + good), (name, form, k, got[:5])
                assert got.final_cost == cost and got.x.tobytes() == np.asarray(x_k, np.float64).tobytes(), (name, form, k)
                assert [r.radius for r in got_trace] == [r.radius for r in trace[:k]]
                assert retries == ref.expected_retries(prob, trace, form, k), (name, form, k)
            else:
                assert same_summary(got, want) and retries == ref.expected_retries(prob, trace, form), (name, form, k)


# ---- 2. scripted mails ---------------------------------------------------------------------------------------------------------
# one attempt's mail, and |x| of the candidate (asked for when the attempt is accepted)
Mail = namedtuple("Mail", "fail model_change step_norm cand_cost cand_gmax x_norm", defaults=(0, 1.0, 1.0, 0.5, 1.0, 1.0))
Cfg = namedtuple("Cfg", "cost gmax x_norm max_iterations radius0 dense_radius dense ns", defaults=(1.0, 1.0, 1.0, 50, -1, 7, 0, 14))
ACCEPT = Mail()                                    # rho = 0.5: the radius stays
REJECT = Mail(cand_cost=2.0)                       # rho = -1
BAD = Mail(fail=1)
FILL = Mail(cand_cost=NAN, model_change=NAN)       # what an attempt nobody judges may hold
Attempt = namedtuple("Attempt", "action verdict radius")  # action "E" / "D", verdict of VERDICT, the radius the step was taken at


def expected(script, cfg, fault=None):
    """the decisions restated (the immediate form) over a script of mails, one per attempt -> (attempts, summary, radius, decrease).
    fault: ONE deliberate mistake - "rho_ge": >= for > at the rho test; "gradient_first": the gradient test in front of the
    iteration limit; "no_reset": `decrease` not reset by an accepted step"""
    cost, gmax, x_norm = cfg.cost, cfg.gmax, cfg.x_norm
    radius, decrease = (1e4 if cfg.radius0 == -1 else 10.0 ** cfg.radius0), 2.0
    use_elim = not cfg.dense and cfg.ns >= 4
    s = dict(initial_cost=cost, final_cost=cost, iterations=0, successful_steps=0, unsuccessful_steps=0, termination=1, n_linearizations=1,
             n_cost_evaluations=0, first_step0=0.0, retries=0.0)
    attempts, mails, invalid_run, first = [], iter(script), 0, False
    accept = (lambda rho: rho >= 1e-3) if fault == "rho_ge" else (lambda rho: rho > 1e-3)
    invalid = lambda m: bool(m.fail) or not m.model_change > 0 or not math.isfinite(m.step_norm)
    if gmax <= 1e-10:
        s["termination"] = 0
        return attempts, s, radius, decrease
    while True:
        limit, small = s["iterations"] >= cfg.max_iterations, gmax <= 1e-10 or radius <= 1e-32
        if limit or small:
            s["termination"] = (0 if small else 1) if fault == "gradient_first" else (1 if limit else 0)
            break
        s["iterations"] += 1
        elim = use_elim and not (cfg.dense_radius > 0 and radius > 10.0 ** cfg.dense_radius)
        m = next(mails)
        s["n_cost_evaluations"] += 1
        if elim:
            rejected = (not invalid(m) and m.step_norm > 1e-8 * (x_norm + 1e-8) and abs(cost - m.cand_cost) > 1e-6 * cost
                        and not accept((cost - m.cand_cost) / m.model_change))
            if invalid(m) or rejected:
                attempts.append(Attempt("E", "R", radius))
                m = next(mails)
                s["n_cost_evaluations"] += 1
                s["retries"] += 1.0
                elim = False
        done = lambda v: attempts.append(Attempt("E" if elim else "D", v, taken_at))
        taken_at = radius
        if invalid(m):
            invalid_run += 1
            if invalid_run >= 5:
                s["termination"] = 2
                done("S")
                break
            radius *= 0.5
            s["unsuccessful_steps"] += 1
            done("x")
            continue
        invalid_run = 0
        if not first:
            first, s["first_step0"] = True, m.step_norm
        if m.step_norm <= 1e-8 * (x_norm + 1e-8) or abs(cost - m.cand_cost) <= 1e-6 * cost:
            s["termination"] = 0
            done("S")
            break
        rho = (cost - m.cand_cost) / m.model_change
        if accept(rho):
            x_norm, cost, gmax = m.x_norm, m.cand_cost, m.cand_gmax
            s["final_cost"] = min(s["final_cost"], cost)
            s["n_linearizations"] += 1
            radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            if fault != "no_reset":
                decrease = 2.0
            s["successful_steps"] += 1
            done("+")
        else:
            radius /= decrease
            decrease *= 2.0
            s["unsuccessful_steps"] += 1
            done("-")
    return attempts, s, radius, decrease


def drive(host, script, cfg, late=False):
    """the script through the header, as wc_window_solve drives it -> (attempts, summary, radius, decrease, late slots read).
    late: the two-collective form - the candidate's max |g| is NOT in the mail that is judged (NaN stands there); it lands in slot
    lin_count & 1 and is handed over with the next attempt's mail"""
    L = Loop(host, cfg.cost, cfg.gmax, cfg.x_norm, cfg.max_iterations, cfg.radius0, cfg.dense_radius, cfg.dense, cfg.ns, int(late))
    attempts, mails, slots, lin_count, read = [], iter(script), [NAN, NAN], 1, []
    assert not L["late_pending"]

    def attempt():
        nonlocal lin_count
        m = next(mails, FILL)
        slot, lin_count = lin_count & 1, lin_count + 1
        late_gmax = NAN
        if L["late_pending"]:
            read.append(int(L["late_at"]))
            late_gmax = slots[read[-1]]
        if late:
            slots[slot] = m.cand_gmax  # (written behind the mail: the judge of THIS attempt was handed the slot's earlier value)
        return m, slot, L.judge(m.fail, m.model_change, m.step_norm, m.cand_cost, NAN if late else m.cand_gmax, late_gmax)

    while True:
        act = L.next()
        if act == STOP:
            break
        radius = L["radius"]
        m, slot, v = attempt()
        if v == RETRY:
            assert act == ELIMINATION
            attempts.append(Attempt("E", "R", radius))
            act = DENSE
            m, slot, v = attempt()
            assert v != RETRY  # (asked for once per iteration)
        attempts.append(Attempt("E" if act == ELIMINATION else "D", VERDICT[v], radius))
        if v == ACCEPTED:
            best = L.accepted(m.x_norm, slot)
            assert best == (L["min_cost"] == L["cost"] == m.cand_cost)
            assert bool(L["late_pending"]) == late and (not late or int(L["late_at"]) == slot)
    assert L.next() == STOP  # (and stays stopped)
    return attempts, L.summary(), L["radius"], L["decrease"], read


def both(host, script, cfg=Cfg()):
    """header and restatement agree on a script -> (attempts, summary, radius, decrease) of the header"""
    got, want = drive(host, script, cfg), expected(script, cfg)
    assert got[0] == want[0], (got[0], want[0])
    assert got[1] == want[1], (got[1], want[1])
    assert got[2:4] == want[2:4], (got[2:4], want[2:4])
    return got[:4]


def verdicts(attempts):
    return "".join(a.verdict for a in attempts)


def tolerance_mails():
    """(step_norm at the parameter tolerance, cand_cost at the function tolerance) for Cfg(cost=1e6, x_norm=3.0)"""
    step = 1e-8 * (3.0 + 1e-8)
    assert 1e-6 * 1e6 == 1.0  # |cost_change| == 1e-6 cost exactly at cand_cost = cost - 1
    return step, 1e6 - 1.0


def mc_for_rho(dc, rho):
    """a model_change with dc / model_change == rho exactly, and the next one below it (a rho above)"""
    mc = dc / rho
    for _ in range(64):
        if dc / mc == rho:
            break
        mc = math.nextafter(mc, INF if dc / mc > rho else 0.0)
    assert dc / mc == rho
    lo = mc
    while dc / lo == rho:
        lo = math.nextafter(lo, 0.0)
    assert dc / lo > rho
    return mc, lo


def above_switch_by_one_ulp(exp=7):
    """a mail accepted at radius 10^exp whose new radius is the next double above it (a rho just above 0.5), found by the recurrence"""
    r0 = 10.0 ** exp
    for i in range(1, 400):
        cand = 0.5 - i * 2.0 ** -20
        rho = (1.0 - cand) / 1.0
        if min(1e16, r0 / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3)) == up(r0):
            return Mail(cand_cost=cand)
    raise AssertionError("no such rho")


RHO_MC, RHO_MC_ABOVE = mc_for_rho(0.5, 1e-3)
P_STEP, F_COST = tolerance_mails()
TOL = Cfg(cost=1e6, x_norm=3.0)
ABOVE = above_switch_by_one_ulp()
# every script of this file, by name: (cfg, mails) - the fault test and the late-form test run all of them
SCRIPTS = {
    "accept_then_gradient": (Cfg(), [ACCEPT, Mail(cand_cost=0.25, cand_gmax=1e-10), ACCEPT]),
    "gradient_above": (Cfg(), [ACCEPT, Mail(cand_cost=0.25, cand_gmax=up(1e-10)), Mail(cand_cost=0.25)]),
    "begin_at_tolerance": (Cfg(gmax=1e-10), [ACCEPT]),
    "begin_above_tolerance": (Cfg(gmax=up(1e-10)), [Mail(cand_cost=1.0)]),
    "limit_0": (Cfg(max_iterations=0), [ACCEPT]),
    "limit_0_at_tolerance": (Cfg(max_iterations=0, gmax=1e-10), [ACCEPT]),
    "limit_1": (Cfg(max_iterations=1), [ACCEPT, ACCEPT]),
    "limit_3": (Cfg(max_iterations=3), [ACCEPT, REJECT, REJECT, REJECT, REJECT, ACCEPT]),
    "limit_before_gradient": (Cfg(max_iterations=2), [ACCEPT, Mail(cand_cost=0.25, cand_gmax=0.0), ACCEPT]),
    "five_invalid": (Cfg(dense=1), [BAD] * 6),
    "five_invalid_elimination": (Cfg(), [BAD] * 12),
    "four_invalid_then_valid": (Cfg(dense=1), [BAD] * 4 + [ACCEPT] + [BAD] * 4 + [Mail(cand_cost=0.25, model_change=0.5)] + [BAD] * 5),
    "parameter_at": (TOL, [Mail(step_norm=P_STEP, cand_cost=5e5)]),
    "parameter_above": (TOL, [Mail(step_norm=up(P_STEP), cand_cost=5e5, model_change=1e6), Mail(cand_cost=5e5)]),
    "function_at": (TOL, [Mail(cand_cost=F_COST)]),
    "function_above": (TOL, [Mail(cand_cost=math.nextafter(F_COST, 0.0)), Mail(cand_cost=F_COST)]),
    "function_at_increase": (TOL, [Mail(cand_cost=1e6 + 1.0)]),
    "rho_at": (Cfg(dense=1), [Mail(model_change=RHO_MC), Mail(cand_cost=1.0)]),
    "rho_at_elimination": (Cfg(), [Mail(model_change=RHO_MC), Mail(model_change=RHO_MC), Mail(cand_cost=1.0)]),
    "rho_above": (Cfg(dense=1), [Mail(model_change=RHO_MC_ABOVE), Mail(cand_cost=0.5)]),
    "rejections_to_the_floor": (Cfg(dense=1), [REJECT] * 40),
    "rejections_to_the_floor_elimination": (Cfg(), [REJECT] * 80),
    "decrease_reset": (Cfg(dense=1), [REJECT, REJECT, ACCEPT, Mail(cand_cost=2.0), Mail(cand_cost=2.0), Mail(cand_cost=0.5)]),
    "cap": (Cfg(cost=8.0, radius0=15, dense_radius=0), [Mail(cand_cost=4.0, model_change=4.0), Mail(cand_cost=2.0, model_change=2.0), Mail(cand_cost=1.0), Mail(cand_cost=1.0)]),
    "switch_at": (Cfg(radius0=7), [REJECT, REJECT, Mail(cand_cost=1.0)]),
    "switch_above": (Cfg(radius0=7), [ABOVE, REJECT, REJECT, REJECT, Mail(cand_cost=ABOVE.cand_cost)]),
    "switch_never": (Cfg(radius0=16, dense_radius=0), [REJECT, REJECT, Mail(cand_cost=1.0)]),
    "switch_ns3": (Cfg(ns=3), [REJECT, BAD, Mail(cand_cost=1.0)]),
    "switch_lm_dense": (Cfg(dense=1), [REJECT, BAD, Mail(cand_cost=1.0)]),
    "retry_second_mail_judged": (Cfg(), [REJECT, Mail(cand_cost=0.75, x_norm=2.0), BAD, Mail(cand_cost=0.5, x_norm=3.0), Mail(cand_cost=0.5)]),
    "retry_not_on_tolerance": (TOL, [Mail(cand_cost=5e5, x_norm=3.0), Mail(step_norm=P_STEP, cand_cost=4e5)]),
    "radius0_default": (Cfg(), [Mail(cand_cost=1.0)]),
    "radius0_10": (Cfg(radius0=10), [REJECT, Mail(cand_cost=1.0)]),
    "late_at_the_floor": (Cfg(radius0=-31, dense=1), [REJECT, REJECT, Mail(cand_cost=1.0 - 0.01, cand_gmax=1e-10), ACCEPT]),
    "late_at_the_floor_above": (Cfg(radius0=-31, dense=1), [REJECT, REJECT, Mail(cand_cost=1.0 - 0.01), ACCEPT]),
}


def run(host, name):
    cfg, script = SCRIPTS[name]
    return both(host, script, cfg)


def test_gradient_tolerance(host):
    a, s, _, _ = run(host, "begin_at_tolerance")  # exactly 1e-10 at begin: no iteration
    assert a == [] and (s["iterations"], s["termination"], s["n_linearizations"], s["n_cost_evaluations"]) == (0, 0, 1, 0)
    assert s["final_cost"] == s["initial_cost"] == 1.0
    a, s, _, _ = run(host, "begin_above_tolerance")  # one ulp above: the loop runs (and ends on the function tolerance)
    assert verdicts(a) == "S" and (s["iterations"], s["termination"]) == (1, 0)
    a, s, _, _ = run(host, "accept_then_gradient")  # after an accepted step
    assert verdicts(a) == "++" and (s["iterations"], s["successful_steps"], s["termination"], s["final_cost"]) == (2, 2, 0, 0.25)
    a, s, _, _ = run(host, "gradient_above")
    assert verdicts(a) == "++S" and s["iterations"] == 3


def test_max_iterations(host):
    a, s, _, _ = run(host, "limit_0")
    assert a == [] and (s["iterations"], s["termination"]) == (0, 1)
    _, s, _, _ = run(host, "limit_0_at_tolerance")  # (Begin's gradient test is in front of the loop, as it always was)
    assert (s["iterations"], s["termination"]) == (0, 0)
    a, s, _, _ = run(host, "limit_1")
    assert verdicts(a) == "+" and (s["iterations"], s["termination"], s["n_linearizations"]) == (1, 1, 2)
    a, s, _, _ = run(host, "limit_3")  # (rejections at 1e4 come from the elimination: each is formed again)
    assert verdicts(a) == "+R-R-" and (s["iterations"], s["successful_steps"], s["unsuccessful_steps"], s["termination"]) == (3, 1, 2, 1)
    a, s, _, _ = run(host, "limit_before_gradient")  # gradient 0 at the limit: the limit is tested first
    assert verdicts(a) == "++" and (s["iterations"], s["termination"]) == (2, 1)


def test_invalid_steps(host):
    a, s, radius, _ = run(host, "five_invalid")
    assert verdicts(a) == "xxxxS" and (s["iterations"], s["unsuccessful_steps"], s["termination"]) == (5, 4, 2)
    assert radius == 1e4 / 16 and [x.radius for x in a] == [1e4 / 2 ** i for i in range(5)]
    assert s["first_step0"] == 0.0 and s["n_linearizations"] == 1 and s["final_cost"] == 1.0
    a, s, radius, _ = run(host, "five_invalid_elimination")  # every invalid elimination step is formed again, and judged once
    assert verdicts(a) == "RxRxRxRxRS" and (s["iterations"], s["unsuccessful_steps"], s["termination"], s["retries"]) == (5, 4, 2, 5.0)
    assert s["n_cost_evaluations"] == 10 and radius == 1e4 / 16
    a, s, radius, _ = run(host, "four_invalid_then_valid")  # a valid step resets the count
    assert verdicts(a) == "xxxx+xxxx+xxxxS" and (s["iterations"], s["unsuccessful_steps"], s["termination"]) == (15, 12, 2)
    assert radius == 1e4 / 2 ** 12


@pytest.mark.parametrize("mail", [Mail(fail=1), Mail(model_change=0.0), Mail(model_change=-1.0), Mail(model_change=NAN),
                                  Mail(step_norm=INF), Mail(step_norm=NAN), Mail(fail=3)])
def test_each_cause_of_invalidity(host, mail):
    a, s, radius, _ = both(host, [mail, ACCEPT, Mail(cand_cost=0.5)], Cfg(dense=1))
    assert verdicts(a) == "x+S" and radius == 5e3 and (s["unsuccessful_steps"], s["successful_steps"]) == (1, 1)
    a, s, _, _ = both(host, [mail, mail, ACCEPT, Mail(cand_cost=0.5)], Cfg())  # from the elimination: formed again first
    assert verdicts(a) == "Rx+S" and s["retries"] == 1.0 and s["n_cost_evaluations"] == 4


def test_tolerances_at_equality_and_one_ulp_above(host):
    a, s, _, _ = run(host, "parameter_at")
    assert verdicts(a) == "S" and (s["iterations"], s["termination"], s["first_step0"]) == (1, 0, P_STEP)
    a, s, _, _ = run(host, "parameter_above")
    assert verdicts(a) == "+S" and s["first_step0"] == up(P_STEP)
    a, s, _, _ = run(host, "function_at")
    assert verdicts(a) == "S" and (s["iterations"], s["successful_steps"], s["termination"], s["final_cost"]) == (1, 0, 0, 1e6)
    a, s, _, _ = run(host, "function_above")
    assert verdicts(a) == "+S" and s["successful_steps"] == 1
    a, s, _, _ = run(host, "function_at_increase")  # (|cost change|: an increase of that size ends the solve as well)
    assert verdicts(a) == "S" and s["termination"] == 0


def test_rho_at_the_threshold_is_a_rejection(host):
    assert 0.5 / RHO_MC == 1e-3 and 0.5 / RHO_MC_ABOVE == up(1e-3)
    a, s, radius, decrease = run(host, "rho_at")
    assert verdicts(a) == "-S" and (radius, decrease, s["unsuccessful_steps"]) == (5e3, 4.0, 1)
    a, s, _, _ = run(host, "rho_at_elimination")  # ... and "about to be rejected" for the re-try
    assert verdicts(a) == "R-S" and s["retries"] == 1.0
    a, s, _, _ = run(host, "rho_above")
    assert verdicts(a) == "+S" and s["successful_steps"] == 1


def test_rejections_down_to_the_radius_floor(host):
    """the exit no window reaches: a run of rejections divides the radius by 2, 4, 8, ... until it is at or below 1e-32"""
    radii, r, d = [], 1e4, 2.0
    while r > 1e-32:
        radii.append(r)
        r, d = r / d, d * 2.0
    assert len(radii) == 15 and r <= 1e-32 < radii[-1]
    a, s, radius, decrease = run(host, "rejections_to_the_floor")
    assert verdicts(a) == "-" * 15 and [x.radius for x in a] == radii and (radius, decrease) == (r, 2.0 ** 16)
    assert (s["iterations"], s["successful_steps"], s["unsuccessful_steps"], s["termination"]) == (15, 0, 15, 0)
    assert s["n_cost_evaluations"] == 15 and s["final_cost"] == 1.0
    a, s, radius, _ = run(host, "rejections_to_the_floor_elimination")  # every one formed again: the radius never exceeds the switch
    assert verdicts(a) == "R-" * 15 and (s["iterations"], s["termination"], s["retries"], s["n_cost_evaluations"]) == (15, 0, 15.0, 30)
    assert [x.radius for x in a[1::2]] == radii and radius == r


def test_an_acceptance_resets_decrease(host):
    a, _, radius, decrease = run(host, "decrease_reset")
    assert verdicts(a) == "--+--S" and [x.radius for x in a] == [1e4, 5e3, 1250.0, 1250.0, 625.0, 156.25] and decrease == 8.0


def test_the_radius_cap(host):
    a, _, radius, _ = run(host, "cap")  # rho = 1: the radius divided by 1 / 3, up to 1e16
    r = [x.radius for x in a]
    assert verdicts(a) == "+++S" and r[:2] == [1e15, 1e15 / (1.0 / 3.0)] and r[2] == r[1] / (1.0 / 3.0) and r[2] / (1.0 / 3.0) > 1e16
    assert r[3] == radius == 1e16


def test_the_switch_to_the_dense_step(host):
    a, s, _, _ = run(host, "switch_at")  # radius == 1e7 exactly: the elimination (and so its re-tries)
    assert a[0] == Attempt("E", "R", 1e7) and a[1] == Attempt("D", "-", 1e7) and s["retries"] == 1.0
    a, s, _, _ = run(host, "switch_above")  # the next double above: the dense step, judged as it comes
    assert a[0] == Attempt("E", "+", 1e7) and a[1] == Attempt("D", "-", up(1e7)) and a[2] == Attempt("E", "R", up(1e7) / 2)
    assert verdicts(a) == "+-R-S" and s["retries"] == 1.0 and s["n_cost_evaluations"] == 5
    a, s, _, _ = run(host, "switch_never")  # option 0
    assert [x.action for x in a] == ["E", "D", "E"] and a[0].radius == 1e16 and s["retries"] == 1.0
    for name in ("switch_ns3", "switch_lm_dense"):  # three sample states, lm_dense = 1: never the elimination
        a, s, _, _ = run(host, name)
        assert [x.action for x in a] == ["D", "D", "D"] and verdicts(a) == "-xS" and s["retries"] == 0.0 and s["n_cost_evaluations"] == 3


def test_the_dense_retry(host):
    a, s, _, _ = run(host, "retry_second_mail_judged")
    # a rejected elimination step whose dense form is accepted; an invalid one whose dense form is accepted; an accepted one: no re-try
    assert [tuple(x[:2]) for x in a] == [("E", "R"), ("D", "+"), ("E", "R"), ("D", "+"), ("E", "S")]
    assert (s["retries"], s["n_cost_evaluations"], s["successful_steps"], s["unsuccessful_steps"], s["final_cost"]) == (2.0, 5, 2, 0, 0.5)
    L = Loop(host, 1.0, 1.0, 1.0)
    assert L.next() == ELIMINATION and L.judge(*REJECT[:5]) == RETRY and L.judge(0, 1.0, 1.0, 0.75, 0.125) == ACCEPTED
    assert L.accepted(2.0) and (L["cost"], L["gmax"], L["x_norm"], L["min_cost"]) == (0.75, 0.125, 2.0, 0.75)  # the second mail's
    a, s, _, _ = run(host, "retry_not_on_tolerance")  # an elimination attempt that ends on a tolerance is not formed again
    assert [tuple(x[:2]) for x in a] == [("E", "+"), ("E", "S")] and s["retries"] == 0.0 and s["termination"] == 0


def test_lm_radius0(host):
    a, _, _, _ = run(host, "radius0_default")
    assert a[0].radius == 1e4
    a, _, _, _ = run(host, "radius0_10")
    assert a[0] == Attempt("D", "-", 1e10) and a[1].radius == 5e9  # (above the switch: the dense step)
    for e in (-31, 0, 3, 16):
        assert Loop(host, 1.0, 1.0, 1.0, radius0=e)["radius"] == 10.0 ** e


def test_first_step_is_recorded_once(host):
    L = Loop(host, 1.0, 1.0, 1.0, dense=1)
    L.next(), L.judge(*BAD[:5])
    assert not L["first_step_now"] and not L["first_recorded"]
    L.next(), L.judge(0, 1.0, 0.375, 2.0, 1.0)  # a rejected step is a valid one
    assert L["first_step_now"] and L["first_step0"] == 0.375
    L.next(), L.judge(0, 1.0, 0.5, 0.5, 1.0)
    assert not L["first_step_now"] and L["first_step0"] == 0.375


# ---- 3. the late gradient ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(SCRIPTS))
def test_late_form_equals_the_immediate_form(host, name):
    cfg, script = SCRIPTS[name]
    now, late = drive(host, script, cfg), drive(host, script, cfg, late=True)
    assert late[1] == now[1], (name, late[1], now[1])  # the summaries, field by field (iterations and n_cost_evaluations among them)
    assert late[2:4] == now[2:4]
    # one more attempt exactly when an accepted point's gradient is at or below the tolerance and the immediate form stops on it
    stops_on_gradient = (verdicts(now[0]).endswith("+") and now[1]["termination"] == 0 and now[1]["iterations"] < cfg.max_iterations
                         and now[2] > 1e-32)
    assert late[0][:len(now[0])] == now[0] and len(late[0]) == len(now[0]) + (1 if stops_on_gradient else 0), (name, late[0], now[0])
    if stops_on_gradient:
        assert late[0][-1].verdict == "S"
    assert now[4] == []  # the immediate form never reads a late slot


def test_late_form_cases(host):
    a = drive(host, *SCRIPTS["accept_then_gradient"][::-1], late=True)
    assert verdicts(a[0]) == "++S" and (a[1]["iterations"], a[1]["n_cost_evaluations"], a[1]["termination"]) == (2, 2, 0)
    # pending at the iteration limit: termination 1 in both forms; pending at the radius floor: 0 in both
    for name, want in (("limit_before_gradient", 1), ("limit_1", 1), ("late_at_the_floor", 0), ("late_at_the_floor_above", 0)):
        cfg, script = SCRIPTS[name]
        now, late = drive(host, script, cfg), drive(host, script, cfg, late=True)
        assert now[1]["termination"] == late[1]["termination"] == want and late[0] == now[0], name
        assert verdicts(now[0]).endswith("+")  # (the accepted point's gradient was still pending when the loop ended)
    assert drive(host, *SCRIPTS["late_at_the_floor"][::-1])[2] <= 1e-32
    # the slot the caller is told to read: where the accepted candidate's linearisation put it - linearisation count & 1, re-tries counted
    cfg, script = SCRIPTS["retry_second_mail_judged"]
    late = drive(host, script, cfg, late=True)
    assert verdicts(late[0]) == "R+R+S" and late[4] == [0, 0]  # (both accepted candidates were the second linearisation of their iteration)
    halves = [Mail(cand_cost=0.5), Mail(cand_cost=0.25, model_change=0.5), Mail(cand_cost=0.125, model_change=0.25)]
    late = drive(host, halves + [REJECT, Mail(cand_cost=0.125)], Cfg(dense=1), late=True)
    assert verdicts(late[0]) == "+++-S" and late[4] == [1, 0, 1]  # the candidates of linearisations 1, 2, 3 were accepted: slots 1, 0, 1 in turn


# ---- 4. deliberate faults ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fault", ["rho_ge", "gradient_first", "no_reset"])
def test_each_mistake_is_caught_by_a_script(host, fault):
    caught = []
    for name, (cfg, script) in SCRIPTS.items():
        got = drive(host, script, cfg)[:4]
        assert got == expected(script, cfg)  # (the restatement without a mistake agrees)
        try:
            wrong = expected(script, cfg, fault)
        except StopIteration:  # the mistaken loop asked for more attempts than the script holds
            wrong = None
        if wrong != got:
            caught.append(name)
    print(fault, "caught by", caught)
    assert caught
    assert {"rho_ge": "rho_at", "gradient_first": "limit_before_gradient", "no_reset": "decrease_reset"}[fault] in caught
