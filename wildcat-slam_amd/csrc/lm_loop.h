// lm_loop.h — the decisions of the window solver's Levenberg-Marquardt loop as plain C++17 (no HIP: g++ compiles it for the CPU
// tests, host/odom_c_api.cc: wc_host_lm_loop).  Ceres' trust-region loop restated (upstream semantics, see oracle/window.cc for the
// per-rule citations) - iteration limit, gradient tolerance, radius floor, HandleInvalidStep up to five in a row, parameter and
// function tolerance, the rho > 1e-3 acceptance, the radius / decrease recurrence, min_cost - plus the project's own rules: the
// lm_dense_radius switch, the dense re-try of an elimination step that is invalid or about to be rejected, and the late max |g| of
// the two-collective sharded form.  wc_window_solve (window.hip) only enqueues what this header decides.
//
// The caller's contract:
//   LmLoop L = lm_begin(cfg, cost, max |g|, |x|)            of the first linearisation
//   while ((a = lm_next(L)) != kLmStop) {
//     enqueue ONE attempt at L.radius from the current point - a == kLmElimination: the bias elimination, kLmDense: the dense
//     factor of all unknowns -, the candidate's linearisation into the other buffer, and wait for its mail
//     v = lm_judge(L, mail)                                 (mail.late_gmax: the late slot L.late_at, read only while L.late_pending)
//     kLmRetryDense   form the step again by the dense factor from the SAME point and radius, wait, and judge that mail instead
//                     (asked for at most once per iteration, and only after kLmElimination)
//     kLmInvalid      nothing: the radius is halved, the next iteration starts from the same point
//     kLmRejected     nothing: the radius shrinks, the candidate and its linearisation are dropped
//     kLmStop         nothing: lm_next returns kLmStop from now on
//     kLmAccepted     swap point and candidate, make the candidate's linearisation the current one, then
//                     lm_accepted(L, |x| of the new point, the late slot this candidate's max |g| lands in): true = the new
//                     point is the best so far and the caller keeps a copy of it
//     whatever v is: L.first_step_now says that this mail held the solve's first valid step (summary.first_step[0] is set; the
//     caller may want the step itself)
//   }
//   lm_summary(L)                                           iterations, final_cost = the best point's, counters, termination
// The late form (cfg.late_gradient): max |g| of an accepted point is not in the mail that accepts it; it arrives with the NEXT
// attempt's mail, in the slot named to lm_accepted.  lm_next does not test the gradient while it is pending, lm_judge looks at it
// first and - at or below the tolerance - takes the attempt back (--iter, not counted): the summary equals the immediate form's.
// No allocation, no globals: the state is a POD the caller owns.  Every expression keeps the form and order it had inside
// wc_window_solve; both builds compile with -ffp-contract=off, so g++ and hipcc take the same decisions on the same doubles.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/wc_types.h"

struct LmConfig {
  int max_iterations;   // wc_params.max_iterations
  int lm_radius0;       // development option: exponent of the first radius, -1 = Ceres' 1e4
  int lm_dense_radius;  // development option: iterations at a radius above 10^this take the dense step; 0 = never
  bool lm_dense;        // development option: every step by the dense factor
  int ns;               // sample states (the bias elimination needs two super-blocks: ns >= 4)
  bool late_gradient;   // the two-collective sharded form
};
inline bool lm_uses_elimination(const LmConfig &c) { return !c.lm_dense && c.ns >= 4; }

enum LmAction { kLmStop = 0, kLmElimination = 1, kLmDense = 2 };
enum LmVerdict { kLmStopped = 0, kLmRetryDense = 1, kLmInvalid = 2, kLmAccepted = 3, kLmRejected = 4 };

// one attempt's mail
struct LmMail {
  int fail;             // the factorisation's fail flag
  double model_change;  // model cost change of the step
  double step_norm;
  double cand_cost, cand_gmax;  // cost and max |g| at the candidate (cand_gmax: not there yet in the late form)
  double late_gmax;     // the late slot's value (looked at only while late_pending)
};

struct LmLoop {
  // configuration
  int max_iterations;
  bool use_elimination, late_gradient;
  double dense_above;  // the radius above which an iteration takes the dense step; 0 = never
  // state
  double cost, gmax, min_cost, radius, decrease, x_norm;
  int iter, consecutive_invalid;
  bool first_recorded, first_step_now;
  bool late_pending;  // max |g| of the accepted point has not been looked at yet: it sits in late slot late_at
  int late_at;
  bool stopped;
  bool elimination_now;  // the attempt to be judged came from the bias elimination
  double rho, cand_cost, cand_gmax;  // of the step lm_judge accepted, for lm_accepted
  wc_solve_summary s;    // (iterations and final_cost: lm_summary)
};

inline LmLoop lm_begin(const LmConfig &c, double cost, double gmax, double x_norm) {
  LmLoop L{};
  L.max_iterations = c.max_iterations;
  L.use_elimination = lm_uses_elimination(c), L.late_gradient = c.late_gradient;
  L.dense_above = c.lm_dense_radius > 0 ? std::pow(10.0, (double)c.lm_dense_radius) : 0.0;
  L.cost = cost, L.gmax = gmax, L.min_cost = cost, L.x_norm = x_norm;
  L.radius = c.lm_radius0 == -1 ? 1e4 : std::pow(10.0, (double)c.lm_radius0), L.decrease = 2.0;
  L.s.n_linearizations = 1;
  L.s.initial_cost = cost;
  L.s.termination = 1;
  if (gmax <= 1e-10) L.s.termination = 0, L.stopped = true;  // GradientToleranceReached before any step
  return L;
}

inline LmAction lm_next(LmLoop &L) {
  if (L.stopped) return kLmStop;
  L.stopped = true;
  if (L.iter >= L.max_iterations) {
    L.s.termination = 1;
    return kLmStop;
  }
  if ((!L.late_pending && L.gmax <= 1e-10) || L.radius <= 1e-32) {
    L.s.termination = 0;
    return kLmStop;
  }
  L.stopped = false;
  ++L.iter;
  // As the radius grows the damping leaves the bias block T, whose own conditioning (random-walk factors tying neighbouring biases,
  // weak absolute information) then shows: cond(T) grows with the radius, and the cyclic reduction's explicit 12 x 12 inverses lose
  // digits a direct factorisation keeps - its normwise backward error in the bias rows is about cond(T) eps.  Measured on the step
  // itself (tests/test_lm_step_gpu.py): at most 2e-10 up to a radius of 1e7, 1.4e-9 at 1e8, 1.2e-8 at 1e9 (the dense step: 1e-15).
  // First seen in profiles/stress_facade.py on sparse streams (a sweep of 38 iterations for the oracle's 35, states 2.5e-4 apart).
  // Iterations above 1e7 take round 2's dense step (development option lm_dense_radius: the exponent, 0 = never).
  L.elimination_now = L.use_elimination && !(L.dense_above > 0 && L.radius > L.dense_above);
  return L.elimination_now ? kLmElimination : kLmDense;
}

inline LmVerdict lm_judge(LmLoop &L, const LmMail &m) {
  L.first_step_now = false;
  if (L.late_pending) {  // max |g| at the point this iteration started from has arrived with the attempt's mail
    L.gmax = m.late_gmax;
    L.late_pending = false;
    if (L.gmax <= 1e-10) {  // GradientToleranceReached there: the reference stops before this iteration
      --L.iter;
      L.s.termination = 0;
      L.stopped = true;
      return kLmStopped;
    }
  }
  L.s.n_cost_evaluations++;
  const bool invalid = m.fail || !(m.model_change > 0) || !std::isfinite(m.step_norm);
  // A step the trust region is about to REJECT (or an invalid one) that came from the bias elimination is formed again by the dense
  // factorisation of all unknowns before the decision is taken (round 5).  The elimination computes S = P - C^T T^-1 C through a
  // parallel cyclic reduction without pivoting; on ill-conditioned windows (a free gauge held by the IMU factors alone, a large
  // radius, dozens of iterations) its step can be worse than a direct factorisation's - profiles/stress_window.py found solves that
  // rejected steps the oracle (and round 2's dense path) accepted and then needed 38 iterations for the oracle's 27, or hit the
  // iteration limit.  Accepted steps - the rule: all of them in the bench's windows, the odometry step and the facade's stream - cost
  // nothing extra; a genuine rejection costs one dense step.
  if (L.elimination_now) {
    const double dc = L.cost - m.cand_cost;
    const bool rejected = !invalid && m.step_norm > 1e-8 * (L.x_norm + 1e-8) && std::fabs(dc) > 1e-6 * L.cost && !(dc / m.model_change > 1e-3);
    if (invalid || rejected) {
      L.elimination_now = false;
      L.s.first_step[1] += 1.0;  // (dense re-tries of this solve)
      return kLmRetryDense;
    }
  }
  if (invalid) {  // HandleInvalidStep
    if (++L.consecutive_invalid >= 5) {
      L.s.termination = 2;
      L.stopped = true;
      return kLmStopped;
    }
    L.radius *= 0.5;
    L.s.unsuccessful_steps++;
    return kLmInvalid;
  }
  L.consecutive_invalid = 0;
  if (!L.first_recorded) {
    L.first_recorded = L.first_step_now = true;
    L.s.first_step[0] = m.step_norm;
  }
  if (m.step_norm <= 1e-8 * (L.x_norm + 1e-8)) {  // ParameterToleranceReached
    L.s.termination = 0;
    L.stopped = true;
    return kLmStopped;
  }
  const double cost_change = L.cost - m.cand_cost;
  if (std::fabs(cost_change) <= 1e-6 * L.cost) {  // FunctionToleranceReached
    L.s.termination = 0;
    L.stopped = true;
    return kLmStopped;
  }
  const double rho = cost_change / m.model_change;
  if (rho > 1e-3) {  // HandleSuccessfulStep: lm_accepted does the rest once the caller has swapped
    L.rho = rho, L.cand_cost = m.cand_cost, L.cand_gmax = m.cand_gmax;
    return kLmAccepted;
  }
  // HandleUnsuccessfulStep
  L.radius = L.radius / L.decrease;
  L.decrease *= 2;
  L.s.unsuccessful_steps++;
  return kLmRejected;
}

inline bool lm_accepted(LmLoop &L, double x_norm, int late_slot) {
  L.x_norm = x_norm;
  L.cost = L.cand_cost, L.gmax = L.cand_gmax;
  if (L.late_gradient) L.gmax = 1.0, L.late_pending = true, L.late_at = late_slot;  // (not there yet: looked at behind the next attempt's mail)
  const bool best = L.cost < L.min_cost;
  if (best) L.min_cost = L.cost;
  L.s.n_linearizations++;
  L.radius = L.radius / std::max(1.0 / 3.0, 1.0 - std::pow(2.0 * L.rho - 1.0, 3));
  L.radius = std::min(1e16, L.radius);
  L.decrease = 2.0;
  L.s.successful_steps++;
  return best;
}

inline wc_solve_summary lm_summary(const LmLoop &L) {
  wc_solve_summary s = L.s;
  s.iterations = L.iter;
  s.final_cost = L.min_cost;
  return s;
}
