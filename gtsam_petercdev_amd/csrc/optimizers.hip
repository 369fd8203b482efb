// optimizers.hip — the LM, GN and Dogleg drivers on the device pipeline of solver.hip, and their entry points.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <array>
#include <map>
#include <string>
#include <vector>

#include "handle.h"

using namespace gsx;

using namespace gsx;

namespace {

// ---- LM policy (host scalars only) — LevenbergMarquardtOptimizer.cpp:121-308 ---------------------------
struct Trace {
  gsx_lm_result* r;
  void push(double err, double lambda, int acc) {
    if (!r) return;
    if (r->trace_len < r->trace_cap) {
      if (r->trace_error) r->trace_error[r->trace_len] = err;
      if (r->trace_lambda) r->trace_lambda[r->trace_len] = lambda;
      if (r->trace_accepted) r->trace_accepted[r->trace_len] = acc;
    }
    r->trace_len++;
  }
};

// One damped trial on the device + the controller's verdict on it (csrc/lm_policy.cpp: gsx_lm_decide).
gsx_status lm_try_lambda(gsx_context* c, const gsx_lm_params& p, Trace& tr, gsx_lm_result* res, bool* done) {
  // (H was assembled by lm_iterate, once for all the trials of the iteration)
  gsx_status ps = damped_step(c, H_KEEP, p.diagonal_damping, p.min_diagonal, p.max_diagonal, c->lm_lambda);
  if (ps != GSX_OK && ps != GSX_E_INDETERMINATE) return ps;
  // a PCG failure is a failed trial like a failed factorization: counted, and lambda goes up
  const bool pcg_ok = ps == GSX_OK;
  if (!pcg_ok) hipMemsetAsync(c->d_delta.p, 0, (size_t)c->P.tan_size * sizeof(double), c->stream);  // (nothing to retract by)
  dev_linear_error(c, true);
  dev_retract(c, c->d_delta.p);
  dev_error(c, c->d_trial.p, SC_TRIAL_ERR);
  gsx_status st = readback(c);
  if (st != GSX_OK) return st;
  const bool solved = c->use_pcg() ? pcg_ok : factorization_ok(c);
  if (!solved && res) res->n_solve_failures++;
  gsx_lm_state ctl{c->lm_lambda, c->lm_factor, c->lm_error, c->lm_iterations, c->lm_inner};
  gsx_lm_decision d;
  gsx_lm_decide(&p, &ctl, solved, c->h_scalars[SC_LIN0], c->h_scalars[SC_LIND], c->h_scalars[SC_TRIAL_ERR], &d);
  if (p.verbosity >= 1)
    std::printf("%4d %12.6g %12.2e %10.2e %6d\n", c->lm_iterations, d.trial_cost, d.cost_change, d.lambda_tried, d.solved);
  if (d.verdict == GSX_LM_TAKE) c->trial_accepted(true);
  c->lm_lambda = ctl.lambda;
  c->lm_factor = ctl.factor;
  c->lm_error = ctl.cost;
  c->lm_iterations = ctl.outer_iterations;
  c->lm_inner = ctl.inner_iterations;
  tr.push(d.trial_cost, d.lambda_tried, d.verdict == GSX_LM_TAKE ? 1 : (solved ? 0 : -1));
  *done = d.verdict != GSX_LM_RETRY;
  return GSX_OK;
}

gsx_status lm_iterate(gsx_context* c, const gsx_lm_params& p, Trace& tr, gsx_lm_result* res) {
  dev_linearize(c);
  // (a PCG handle reads H only for diag(J'J), the weights of diagonal damping)
  if (!c->use_pcg() || p.diagonal_damping) dev_assemble_h(c);
  bool done = false;
  while (!done) {
    gsx_status st = lm_try_lambda(c, p, tr, res, &done);
    if (st != GSX_OK) return st;
  }
  return GSX_OK;
}

bool check_convergence(double relTol, double absTol, double errTol, double currentError, double newError) {
  if (newError <= errTol) return true;
  const double absoluteDecrease = currentError - newError;
  const double relativeDecrease = absoluteDecrease / currentError;
  return (relTol && (relativeDecrease <= relTol)) || (absoluteDecrease <= absTol);
}

// NonlinearOptimizer::defaultOptimize — gtsam/nonlinear/NonlinearOptimizer.cpp:62-117 — around one optimizer's
// iterate(): the error at the start, the loop, the result.  `iterate(trace)` runs one outer iteration and leaves the new
// error in lm_error and the count in lm_iterations; the caller adds final_lambda / inner_iterations of its own.
template <class Iterate>
gsx_status default_optimize(gsx_context* h, int max_iterations, double relTol, double absTol, double errTol,
                            gsx_lm_result* r, Iterate& iterate) {
  gsx_status st = compute_error_sync(h, &h->lm_error);
  if (st != GSX_OK) return st;
  h->lm_iterations = 0;
  h->pcg_run_iterations = 0;
  Trace tr{r};
  if (r) {
    r->initial_error = h->lm_error;
    r->trace_len = 0;
    r->n_solve_failures = 0;
  }
  double currentError = h->lm_error;
  if (!(currentError <= errTol) && !(h->lm_iterations >= max_iterations)) {
    double newError = currentError;
    do {
      currentError = newError;
      st = iterate(tr);
      if (st != GSX_OK) return st;
      newError = h->lm_error;
    } while (h->lm_iterations < max_iterations && !check_convergence(relTol, absTol, errTol, currentError, newError) &&
             std::isfinite(currentError));
  }
  if (r) {
    r->final_error = h->lm_error;
    r->iterations = h->lm_iterations;
    r->inner_iterations = h->lm_iterations;
    if (h->use_pcg()) r->pcg_iterations = (int32_t)h->pcg_run_iterations;
  }
  return GSX_OK;
}

}  // namespace

extern "C" {

void gsx_lm_params_legacy(gsx_lm_params* p) {
  // LevenbergMarquardtParams::SetLegacyDefaults — LevenbergMarquardtParams.h:69-82
  *p = gsx_lm_params{100, 1e-5, 1e-5, 0.0, 1e-5, 10.0, 1e5, 0.0, 1e-3, 0, 1, 1e-6, 1e32, 0};
}
void gsx_lm_params_ceres(gsx_lm_params* p) {
  // LevenbergMarquardtParams::SetCeresDefaults — LevenbergMarquardtParams.h:85-98
  *p = gsx_lm_params{50, 1e-6, 0.0, 0.0, 1e-4, 2.0, 1e32, 1e-16, 1e-3, 1, 0, 1e-6, 1e32, 0};
}

gsx_status gsx_lm_reset(gsx_handle h, const gsx_lm_params* p) {
  if (!h || !p) return GSX_E_INVALID;
  gsx_status st = begin_call(h, true, false);
  if (st != GSX_OK) return st;
  st = compute_error_sync(h, &h->lm_error);
  if (st != GSX_OK) return st;
  h->lm_lambda = p->lambda_initial;
  h->lm_factor = p->lambda_factor;
  h->lm_iterations = 0;
  h->lm_inner = 0;
  return GSX_OK;
}

gsx_status gsx_lm_iterate(gsx_handle h, const gsx_lm_params* p, double* error, double* lambda) {
  if (!h || !p) return GSX_E_INVALID;
  gsx_status st = begin_call(h, true, true);
  if (st != GSX_OK) return st;
  Trace tr{nullptr};
  st = lm_iterate(h, *p, tr, nullptr);
  if (st != GSX_OK) return st;
  if (error) *error = h->lm_error;
  if (lambda) *lambda = h->lm_lambda;
  return GSX_OK;
}

gsx_status gsx_lm_trial(gsx_handle h, int32_t relinearize, double lambda, int32_t diagonal_damping, double min_diagonal,
                        double max_diagonal, double* lin0, double* lind, double* trial_error) {
  if (!h || !(lambda >= 0.0)) return GSX_E_INVALID;
  gsx_status st = begin_call(h, true, true);
  if (st != GSX_OK) return st;
  if (!relinearize && !h->linearized) {
    h->err = "linearize first";
    return GSX_E_STATE;
  }
  if (relinearize) dev_linearize(h);
  st = damped_step(h, H_IF_STALE, diagonal_damping, min_diagonal, max_diagonal, lambda);
  if (st != GSX_OK) return st;
  dev_linear_error(h, true);
  dev_retract(h, h->d_delta.p);
  dev_error(h, h->d_trial.p, SC_TRIAL_ERR);
  st = readback(h);
  if (st != GSX_OK) return st;
  if (!h->use_pcg()) {   // (PCG judged its own step)
    st = indeterminate(h, nullptr, true);
    if (st != GSX_OK) {
      h->delta_outdated();
      return st;
    }
  }
  h->step_solved(false);
  if (lin0) *lin0 = h->h_scalars[SC_LIN0];
  if (lind) *lind = h->h_scalars[SC_LIND];
  if (trial_error) *trial_error = h->h_scalars[SC_TRIAL_ERR];
  return GSX_OK;
}

gsx_status gsx_lm_optimize(gsx_handle h, const gsx_lm_params* p, gsx_lm_result* r) {
  if (!h || !p) return GSX_E_INVALID;
  gsx_status st = begin_call(h, true, true);
  if (st != GSX_OK) return st;
  h->lm_lambda = p->lambda_initial;   // (gsx_lm_reset: the error and the iteration count are default_optimize's)
  h->lm_factor = p->lambda_factor;
  h->lm_inner = 0;
  auto iterate = [&](Trace& tr) -> gsx_status { return lm_iterate(h, *p, tr, r); };
  st = default_optimize(h, p->max_iterations, p->relative_error_tol, p->absolute_error_tol, p->error_tol, r, iterate);
  if (st == GSX_OK && r) {
    r->final_lambda = h->lm_lambda;
    r->inner_iterations = h->lm_inner;
  }
  return st;
}

// GaussNewtonOptimizer::iterate — gtsam/nonlinear/GaussNewtonOptimizer.cpp:44-66
gsx_status gsx_gn_optimize(gsx_handle h, int32_t max_iterations, double relTol, double absTol, double errTol,
                           gsx_lm_result* r) {
  if (!h) return GSX_E_INVALID;
  gsx_status st = begin_call(h, true, true);
  if (st != GSX_OK) return st;
  auto iterate = [&](Trace& tr) -> gsx_status {
    dev_linearize(h);
    // (PCG: PCGSolver on the undamped graph — NonlinearOptimizer.cpp:154-162 from GaussNewtonOptimizer::iterate)
    gsx_status is = damped_step(h, H_ALWAYS, 0, 0, 0, 0.0);
    if (is != GSX_OK) return is;
    dev_retract(h, h->d_delta.p);
    dev_error(h, h->d_trial.p, SC_TRIAL_ERR);
    is = readback(h);
    if (is != GSX_OK) return is;
    if (!h->use_pcg()) {   // (solved and fact_valid are down already: the linearize, the readback)
      is = indeterminate(h, nullptr, true);
      if (is != GSX_OK) return is;
    }
    h->trial_accepted(false);
    h->lm_error = h->h_scalars[SC_TRIAL_ERR];
    h->lm_iterations++;
    tr.push(h->lm_error, 0.0, 1);
    return GSX_OK;
  };
  st = default_optimize(h, max_iterations, relTol, absTol, errTol, r, iterate);
  if (st == GSX_OK && r) r->final_lambda = 0;
  return st;
}

// DoglegOptimizerImpl::ComputeDoglegPoint coefficients: dx_d = cu dx_u + cn dx_n  (DoglegOptimizerImpl.cpp:26-86)
static void dogleg_coefficients(double delta, double uu, double nn, double un, double* cu, double* cn) {
  const double deltaSq = delta * delta;
  if (deltaSq < uu) {
    *cu = std::sqrt(deltaSq / uu);
    *cn = 0.0;
  } else if (deltaSq < nn) {
    const double a = uu - 2. * un + nn, b = 2. * (un - uu), c = uu - deltaSq;
    const double sq = std::sqrt(b * b - 4 * a * c);
    const double tau1 = (-b + sq) / (2. * a), tau2 = (-b - sq) / (2. * a);
    const double eps = std::numeric_limits<double>::epsilon();
    const double tau = (-eps <= tau1 && tau1 <= 1.0 + eps) ? tau1 : tau2;
    *cu = 1. - tau;
    *cn = tau;
  } else {
    *cu = 0.0;
    *cn = 1.0;
  }
}

gsx_status gsx_dogleg_point(double delta, const double* dx_u, const double* dx_n, int64_t n, double* out) {
  if (!dx_u || !dx_n || !out || n < 0 || !(delta >= 0)) return GSX_E_INVALID;
  double uu = 0, nn = 0, un = 0;
  for (int64_t i = 0; i < n; ++i) {
    uu += dx_u[i] * dx_u[i];
    nn += dx_n[i] * dx_n[i];
    un += dx_u[i] * dx_n[i];
  }
  double cu, cn;
  dogleg_coefficients(delta, uu, nn, un, &cu, &cn);
  for (int64_t i = 0; i < n; ++i) out[i] = (cn == 0.0 ? cu * dx_u[i] : (cu == 0.0 ? dx_n[i] : cu * dx_u[i] + cn * dx_n[i]));
  return GSX_OK;
}

// DoglegOptimizer::iterate (gtsam/nonlinear/DoglegOptimizer.cpp:84-121) with DoglegOptimizerImpl::Iterate in
// ONE_STEP_PER_ITERATION mode (DoglegOptimizerImpl.h:137-252), inside NonlinearOptimizer::defaultOptimize.
// The reference evaluates the model M on the Bayes tree [R S d]; M(0) - M(dx) is the same number on the linearized
// graph it was eliminated from (the two differ by a constant), which is what the device has.
gsx_status gsx_dogleg_optimize(gsx_handle h, double delta_initial, int32_t max_iterations, double relTol, double absTol,
                               double errTol, gsx_lm_result* r) {
  if (!h || !(delta_initial >= 0)) return GSX_E_INVALID;
  gsx_status st = begin_call(h, true, true);
  if (st != GSX_OK) return st;
  if (h->sharded()) {
    h->err = "Dogleg is not available on a sharded handle";
    return GSX_E_STATE;
  }
  if (h->constrained()) {
    // (the steepest-descent leg of the dog leg knows nothing of the constraint rows: a blended step would violate them)
    h->err = "Dogleg is not available on a problem with hard constraints";
    return GSX_E_STATE;
  }
  if (h->use_pcg()) {
    // (the dog leg blends the steepest-descent point with the EXACT Gauss-Newton point of the Bayes tree)
    h->err = "Dogleg is not available on a handle whose linear solver is PCG";
    return GSX_E_STATE;
  }
  const int64_t nt = h->P.tan_size;
  if (!h->d_dlu.p) {
    HIPCHK(h, h->d_dlu.alloc(std::max<int64_t>(nt, 1)));
    HIPCHK(h, h->d_dld.alloc(std::max<int64_t>(nt, 1)));
  }
  double delta = delta_initial;
  auto iterate = [&](Trace& tr) -> gsx_status {
    dev_linearize(h);
    direct_solve(h, H_ALWAYS, 0, 0, 0, 0.0, true);  // d_delta = Newton point dx_n
    dev_ensure_hstar(h);
    // steepest-descent point: grad = -A'b = -g, dx_u = -(grad'grad / |A grad|^2) grad = (g'g / |A g|^2) g
    launch_gradient(h->DP, h->DS, h->d_H.p, h->d_dlu.p, h->stream);
    launch_vec_dot(h->d_dlu.p, h->d_dlu.p, nt, h->d_partials.p, gsx_context::kPartials, h->d_scalars.p, SC_DOT0, h->stream);
    launch_ax_sqnorm(h->DP, h->d_jac.p, h->d_dlu.p, h->d_partials.p, gsx_context::kPartials, h->d_scalars.p, SC_DOT1,
                     h->stream);
    launch_vec_dot(h->d_delta.p, h->d_delta.p, nt, h->d_partials.p, gsx_context::kPartials, h->d_scalars.p, SC_DOT2,
                   h->stream);
    launch_vec_dot(h->d_dlu.p, h->d_delta.p, nt, h->d_partials.p, gsx_context::kPartials, h->d_scalars.p, SC_DOT3,
                   h->stream);
    gsx_status is = readback(h);
    if (is != GSX_OK) return is;
    is = indeterminate(h, nullptr, true);   // (solved and fact_valid are down already: the linearize, the readback)
    if (is != GSX_OK) return is;
    const double gg = h->h_scalars[SC_DOT0], ag2 = h->h_scalars[SC_DOT1];
    const double step = gg / ag2;
    const double uu = step * step * gg, nn = h->h_scalars[SC_DOT2], un = step * h->h_scalars[SC_DOT3];
    const double f_error = h->lm_error;
    double result_f = f_error, cu = 0, cn = 0;
    bool stay = true, zero_step = false;
    while (stay) {
      dogleg_coefficients(delta, uu, nn, un, &cu, &cn);
      launch_vec_axpby(h->d_dld.p, cu * step, h->d_dlu.p, cn, h->d_delta.p, nt, h->stream);  // dx_d (d_dlu holds g)
      dev_retract(h, h->d_dld.p);
      dev_error(h, h->d_trial.p, SC_TRIAL_ERR);
      launch_linear_error(h->DP, h->d_jac.p, h->d_dld.p, h->d_partials.p, gsx_context::kPartials, h->d_scalars.p,
                          h->lin_err_slice, h->stream);
      is = readback(h);
      if (is != GSX_OK) return is;
      result_f = h->h_scalars[SC_TRIAL_ERR];
      const double M_error = h->h_scalars[SC_LIN0], new_M = h->h_scalars[SC_LIND];
      const double rho = (std::abs(f_error - result_f) < 1e-15 || std::abs(M_error - new_M) < 1e-15)
                             ? 0.5
                             : (f_error - result_f) / (M_error - new_M);
      if (rho >= 0.75) {
        const double dnorm = std::sqrt(cu * cu * uu + 2 * cu * cn * un + cn * cn * nn);
        delta = std::max(delta, 3.0 * dnorm);
        stay = false;
      } else if (rho >= 0.25) {
        stay = false;
      } else if (rho >= 0.0) {
        if (delta > 1e-5) delta *= 0.5;
        stay = false;
      } else {  // f increased (NaN lands here too): shrink the region until it does not
        if (delta > 1e-5) {
          delta *= 0.5;
          stay = true;
        } else {
          zero_step = true;  // do not allow the error to increase
          result_f = f_error;
          stay = false;
        }
      }
    }
    if (zero_step) h->trial_discarded();
    else h->trial_accepted(false);
    h->lm_error = result_f;
    h->lm_iterations++;
    tr.push(h->lm_error, delta, 1);  // the trace's "lambda" column carries the trust-region radius
    return GSX_OK;
  };
  st = default_optimize(h, max_iterations, relTol, absTol, errTol, r, iterate);
  if (st == GSX_OK && r) r->final_lambda = delta;
  return st;
}

}  // extern "C"
