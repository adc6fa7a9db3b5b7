// Host-side trust-region loop shared by the Schur and the dense paths: the iteration (step), the control flow of the three
// strategies below it (try_step, line_search), the phase accounting.  A solver supplies device work through linear_solve,
// dogleg_trial and bounded_trial (solver.hpp).
#include "solver.hpp"

#include <cmath>
#include <limits>

namespace sk {

static thread_local std::string g_error;
void set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_error = buf;
}
const char* get_error() { return g_error.c_str(); }
// the status that goes with a failure reported through a null handle (sk_solver_create): typed, not parsed from the text
static thread_local int g_status = SK_OK;
void set_status(int status) { g_status = status; }
int get_status() { return g_status; }

const char* linear_solver_name(int t) {
  switch (t) {
    case SK_DENSE_NORMAL_CHOLESKY: return "DENSE_NORMAL_CHOLESKY";
    case SK_DENSE_QR: return "DENSE_QR";
    case SK_SPARSE_NORMAL_CHOLESKY: return "SPARSE_NORMAL_CHOLESKY";
    case SK_DENSE_SCHUR: return "DENSE_SCHUR";
    case SK_SPARSE_SCHUR: return "SPARSE_SCHUR";
    case SK_ITERATIVE_SCHUR: return "ITERATIVE_SCHUR";
    case SK_CGNR: return "CGNR";
  }
  return "UNKNOWN";
}
const char* termination_name(int t) {
  switch (t) {
    case SK_CONVERGENCE: return "CONVERGENCE";
    case SK_NO_CONVERGENCE: return "NO_CONVERGENCE";
    case SK_FAILURE: return "FAILURE";
    case SK_USER_SUCCESS: return "USER_SUCCESS";
    case SK_USER_FAILURE: return "USER_FAILURE";
  }
  return "UNKNOWN";
}

namespace dogleg {
bool interpolate(const Scalars& k, double radius, double* a, double* b, double* step_norm, double* model_cost_change) {
  if (!(k.w_w > 0.0) || !(k.g_g > 0.0) || !std::isfinite(k.p_p) || !std::isfinite(k.m_m) || !std::isfinite(k.w_w)) return false;
  const double g = std::sqrt(k.g_g), pn = std::sqrt(k.p_p), alpha = k.g_g / k.w_w;
  if (pn <= radius) {  // the Gauss-Newton step lies inside the region
    *a = 0.0; *b = 1.0; *step_norm = pn;
  } else if (alpha * g >= radius) {  // the Cauchy point lies outside: the gradient direction, cut at the boundary
    *a = radius / g; *b = 0.0; *step_norm = radius;
  } else {  // where the segment from the Cauchy point to the Gauss-Newton step leaves the region
    const double a2 = (alpha * g) * (alpha * g), ba = -alpha * k.g_p, bma2 = a2 - 2.0 * ba + k.p_p, c = ba - a2;
    const double d = std::sqrt(c * c + bma2 * (radius * radius - a2));
    const double beta = c <= 0.0 ? (d - c) / bma2 : (radius * radius - a2) / (d + c);
    *a = alpha * (1.0 - beta); *b = beta;
    *step_norm = std::sqrt(*a * *a * k.g_g - 2.0 * *a * *b * k.g_p + *b * *b * k.p_p);
  }
  *model_cost_change = -(*a * k.w_r + *b * k.m_r + 0.5 * (*a * *a * k.w_w + 2.0 * *a * *b * k.w_m + *b * *b * k.m_m));
  return std::isfinite(*step_norm) && std::isfinite(*model_cost_change);
}
}  // namespace dogleg

bool SolverBase::strategy_stat(const std::string& name, double* value) const {
  if (name == "bounded_coordinates") { *value = (double)bounded_coordinates_; return true; }
  if (name == "active_bounds") { *value = (double)active_bounds_; return true; }
  if (name == "line_search_evaluations") { *value = (double)n_ls_evals_; return true; }
  if (name == "inner_iteration_steps") { *value = (double)inner_steps_; return true; }
  if (name == "inner_iteration_rounds") { *value = (double)inner_rounds_; return true; }
  if (name == "inner_iterations_enabled") { *value = opt_.use_inner_iterations && inner_enabled_ ? 1.0 : 0.0; return true; }
  if (name == "inner_iteration_seconds") { *value = inner_seconds_; return true; }
  if (name == "linear_solves") { *value = (double)n_linear_solves_; return true; }
  if (name == "dogleg_reused_steps") { *value = (double)n_dl_reused_; return true; }
  if (name == "dogleg_mu") { *value = dl_mu_; return true; }
  if (name.rfind("dogleg_", 0) == 0 && dogleg()) {
    const struct { const char* n; double v; } t[] = {{"dogleg_w_r", dl_k_.w_r}, {"dogleg_m_r", dl_k_.m_r}, {"dogleg_w_w", dl_k_.w_w}, {"dogleg_w_m", dl_k_.w_m},
      {"dogleg_m_m", dl_k_.m_m}, {"dogleg_g_g", dl_k_.g_g}, {"dogleg_g_p", dl_k_.g_p}, {"dogleg_p_p", dl_k_.p_p}, {"dogleg_a", dl_a_}, {"dogleg_b", dl_b_}};
    for (const auto& e : t) if (name == e.n) { *value = e.v; return true; }
  }
  return false;
}

SolverBase::~SolverBase() {
  for (auto& e : ev_) if (e) (void)hipEventDestroy(e);
  for (auto& e : ar_pending_) (void)hipEventDestroy(e);
  for (auto& e : ar_free_) (void)hipEventDestroy(e);
  if (own_stream_ && stream_) (void)hipStreamDestroy(stream_);
}

int SolverBase::init_device() {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    set_error("no HIP device available: libskeres_amd has no CPU fallback");
    return SK_ERR_NO_DEVICE;
  }
  if (opt_.device >= 0) SK_HIP_TRY(hipSetDevice(opt_.device));
  int dev = 0;
  SK_HIP_TRY(hipGetDevice(&dev));
  hipDeviceProp_t prop;
  SK_HIP_TRY(hipGetDeviceProperties(&prop, dev));
  device_name_ = std::string(prop.name) + " (" + prop.gcnArchName + ")";
  if (opt_.stream_set) {
    stream_ = opt_.stream;
  } else {
    SK_HIP_TRY(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    own_stream_ = true;
  }
  for (int i = 0; i < kEvCount; ++i) SK_HIP_TRY(hipEventCreate(&ev_[i]));
  return SK_OK;
}

void SolverBase::add_phase(int i, hipEvent_t from, hipEvent_t to) {
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, from, to) == hipSuccess) phase_[i] += 1e-3 * ms;
  else (void)hipGetLastError();
}
void SolverBase::add_phases(int first, int last, int since) {
  for (int i = first; i <= last; ++i) { add_phase(i, ev_[since], ev_[i + 1]); since = i + 1; }
}

// The hook runs on the solver's stream and the solver goes on enqueueing behind it: NO host synchronisation here (until round 5 every
// collective ended in one — four per iteration of a segmented world, the device idle while the host caught up with its launches).  The
// time of the all-reduce phase comes from event pairs that are read once they have completed (here, opportunistically, and in finish()).
void SolverBase::collect_allreduce_time(bool all) {
  size_t done = 0;
  for (; done + 1 < ar_pending_.size(); done += 2) {
    if (!all && hipEventQuery(ar_pending_[done + 1]) != hipSuccess) { (void)hipGetLastError(); break; }
    if (all) (void)hipEventSynchronize(ar_pending_[done + 1]);
    add_phase(5, ar_pending_[done], ar_pending_[done + 1]);
    ar_free_.push_back(ar_pending_[done]); ar_free_.push_back(ar_pending_[done + 1]);
  }
  ar_pending_.erase(ar_pending_.begin(), ar_pending_.begin() + (long)done);
}

int SolverBase::allreduce(double* dev, size_t count) {
  if (!opt_.allreduce) return SK_OK;  // the hook decides: a world of 1 with a hook still exercises the whole path
  collect_allreduce_time(ar_pending_.size() >= 64);
  hipEvent_t ab[2];
  for (hipEvent_t& e : ab) {
    if (!ar_free_.empty()) { e = ar_free_.back(); ar_free_.pop_back(); }
    else SK_HIP_TRY(hipEventCreate(&e));
  }
  SK_HIP_TRY(hipEventRecord(ab[0], stream_));
  if (opt_.allreduce(opt_.allreduce_user, dev, count, (void*)stream_) != 0) {
    ar_free_.push_back(ab[0]); ar_free_.push_back(ab[1]);
    set_error("allreduce hook failed");
    return SK_ERR_COMM;
  }
  SK_HIP_TRY(hipEventRecord(ab[1], stream_));
  ar_pending_.push_back(ab[0]); ar_pending_.push_back(ab[1]);
  return SK_OK;
}

void SolverBase::log_iteration(int it, double cost_change, double step_norm, double rho, int valid, int success, double iter_time) {
  IterationLog L;
  L.iteration = it; L.cost = cost_; L.cost_change = cost_change; L.gradient_max_norm = gmax_;
  L.step_norm = step_norm; L.relative_decrease = rho; L.trust_region_radius = radius_;
  L.step_is_valid = valid; L.step_is_successful = success; L.iter_time = iter_time; L.total_time = now();
  L.step_size = ls_alpha_; L.line_search_evaluations = ls_evals_;
  L.linear_solver_iterations = it == 0 ? 0 : cg_iterations_last_;
  L.inner_iteration_rounds = it == 0 ? 0 : inner_rounds_last_;
  sum_.iterations.push_back(L);
  if (opt_.progress_to_stdout && opt_.rank == 0) {
    if (it == 0) printf("iter      cost      cost_change  |gradient|   |step|    tr_ratio  tr_radius  ls_iter  iter_time  total_time\n");
    printf("%4d % 8e   % 3.2e   % 3.2e  % 3.2e  % 3.2e % 3.2e     % 4d   % 3.2e   % 3.2e\n", it, L.cost, L.cost_change,
           L.gradient_max_norm, L.step_norm, L.relative_decrease, L.trust_region_radius, L.line_search_evaluations, L.iter_time, L.total_time);
    fflush(stdout);
  }
}

int SolverBase::create() {
  t0_ = std::chrono::steady_clock::now();
  if (opt_.minimizer_type != SK_TRUST_REGION) { set_error("only TRUST_REGION (Levenberg-Marquardt) is implemented"); return SK_ERR_UNSUPPORTED; }
  if (dogleg()) {
    if (opt_.dogleg_type != SK_TRADITIONAL_DOGLEG) { set_error("SUBSPACE_DOGLEG is not implemented (not supported: TRADITIONAL_DOGLEG is)"); return SK_ERR_UNSUPPORTED; }
    if (opt_.world > 1) { set_error("DOGLEG is implemented for one device (not supported in a world of %d ranks)", opt_.world); return SK_ERR_UNSUPPORTED; }
    if (!supports_dogleg()) { set_error("DOGLEG is implemented for DENSE_SCHUR and for DENSE_QR / DENSE_NORMAL_CHOLESKY over residual blocks (not supported on dense-row problems)"); return SK_ERR_UNSUPPORTED; }
  }
  sum_.trust_region_strategy_type = opt_.trust_region_strategy_type;
  int rc = check_bounds();
  if (rc) return rc;
  if (infeasible_) return SK_OK;
  rc = init_device();
  if (rc) return rc;
  rc = setup();
  if (rc) return rc;
  rc = evaluate_with_jacobian(true);
  if (rc == SK_ERR_EVALUATION_FAILED) {
    sum_.termination_type = SK_FAILURE;
    sum_.message = "Initial residual and Jacobian evaluation failed.";
    terminated_ = true;
    return SK_OK;
  }
  if (rc) return rc;
  sum_.initial_cost = cost_;
  radius_ = opt_.initial_trust_region_radius;
  decrease_factor_ = 2.0;
  iteration_ = 0;
  log_iteration(0, 0.0, 0.0, 0.0, 1, 1, now());
  sum_.termination_type = SK_NO_CONVERGENCE;
  return SK_OK;
}

// Parameter bounds, before anything touches the device: what is refused, and whether the box is feasible (Ceres:
// Problem::IsFeasible in the preprocessor — "lower >= upper" for a variable block, a constant block outside its bounds).
int SolverBase::check_bounds() {
  const Problem& p = *problem_;
  bounded_ = p.has_bounds();
  if (!bounded_) return SK_OK;
  if (dogleg()) { set_error("parameter bounds with DOGLEG are not supported (LEVENBERG_MARQUARDT takes them)"); return SK_ERR_UNSUPPORTED; }
  if (opt_.world > 1) { set_error("parameter bounds are implemented for one device (not supported in a world of %d ranks)", opt_.world); return SK_ERR_UNSUPPORTED; }
  if (const char* why = refuses_bounds()) { set_error("%s", why); return SK_ERR_UNSUPPORTED; }
  char msg[256];
  for (size_t b = 0; b < p.block_ptr.size(); ++b) {
    if (!p.block_has_bounds(b)) continue;
    const int pi = b < p.block_param.size() ? p.block_param[b] : -1;
    if (pi >= 0 && (p.params[pi].type == kParamQuaternion || p.params[pi].type == kParamHomogeneousVector)) {
      set_error("parameter bounds on block %d, which carries a quaternion or homogeneous-vector parameterization, are not supported", (int)b);
      return SK_ERR_UNSUPPORTED;
    }
    const bool constant = b < p.block_constant.size() && p.block_constant[b];
    for (int i = 0; i < p.block_size[b]; ++i) {
      const double lo = p.lower_bound(b, i), hi = p.upper_bound(b, i);
      const bool held = constant || (pi >= 0 && p.params[pi].type == kParamSubset && ((p.params[pi].constant_mask >> i) & 1u));
      if (std::isfinite(lo) || std::isfinite(hi)) ++bounded_coordinates_;
      msg[0] = 0;
      if (held) {
        const double v = p.block_ptr[b][i];
        if (!(v >= lo && v <= hi)) snprintf(msg, sizeof(msg), "Infeasible problem: parameter block %d, index %d is constant at %g outside its bounds [%g, %g].", (int)b, i, v, lo, hi);
      } else if (lo >= hi) {
        snprintf(msg, sizeof(msg), "Infeasible problem: parameter block %d, index %d has lower bound %g >= upper bound %g.", (int)b, i, lo, hi);
      }
      if (msg[0]) { sum_.termination_type = SK_FAILURE; sum_.message = msg; terminated_ = true; infeasible_ = true; return SK_OK; }
    }
  }
  return SK_OK;
}

// The line search of an iteration under bounds (common.hpp: namespace bounds) on phi(alpha) = cost(P(x + alpha delta)), f0 = cost_.
// In: *cost = phi(1) and *step_norm of the candidate the linear solve has formed.  Out: those of the alpha that was kept (ls_alpha_), the
// candidate buffers holding its point.  A search that fails keeps alpha = 1, as Ceres leaves delta alone.
int SolverBase::line_search(double g0, double max_delta, double* cost, double* step_norm) {
  ls_alpha_ = 1.0; ls_evals_ = 1; ++n_ls_evals_;
  if (!(g0 < 0.0) || !std::isfinite(g0)) return SK_OK;
  const double f0 = cost_;
  double alpha = 1.0, phi = *cost, norm = *step_norm;
  bool found = false;
  for (int contractions = 0;; ++contractions) {
    if (std::isfinite(phi) && phi <= f0 + bounds::kSufficientDecrease * alpha * g0) { found = true; break; }
    if (contractions == bounds::kMaxNumIterations) break;
    double next = bounds::kBisection * alpha;
    if (std::isfinite(phi)) {
      next = -g0 * alpha * alpha / (2.0 * (phi - f0 - g0 * alpha));
      next = std::min(std::max(next, bounds::kMaxStepContraction * alpha), bounds::kMinStepContraction * alpha);
    }
    if (next * max_delta < bounds::kMinStepSize) break;
    alpha = next;
    int rc = bounded_trial(alpha, &phi, &norm);
    if (rc) return rc;
    ++ls_evals_; ++n_ls_evals_;
  }
  if (!found && alpha != 1.0) {  // back to the full step: its point into the candidate buffers again
    alpha = 1.0;
    int rc = bounded_trial(alpha, &phi, &norm);
    if (rc) return rc;
    ++ls_evals_; ++n_ls_evals_;
  }
  ls_alpha_ = alpha; *cost = phi; *step_norm = norm;
  return SK_OK;
}

// One candidate for this radius: valid (a step could be formed), the model's cost change, the candidate's cost, |x - candidate|.
// Levenberg-Marquardt: one linear solve, the candidate and its cost fused into it.  Bounds: the same solve — the unconstrained step
// and its model — then the line search over P(x + alpha delta).  DOGLEG: after a new Jacobian the Gauss-Newton solve at the current
// mu, again at ten times mu while the damped system is not positive definite (each solve counts in "linear_solves"); then, and
// after every rejected step (dl_reuse_), the candidate of this radius from the two vectors the solve left on the device.
int SolverBase::try_step(double radius, bool* valid, double* model_cost_change, double* new_cost, double* step_norm) {
  *valid = false;
  LinearSolve solve;
  if (!dogleg()) {
    int rc = linear_solve(radius, &solve);
    if (rc || !solve.valid) return rc;
    *valid = true;
    *model_cost_change = solve.model_cost_change; *new_cost = solve.cost; *step_norm = solve.step_norm;
    return bounded_ ? line_search(solve.g_delta, solve.max_delta, new_cost, step_norm) : SK_OK;
  }
  if (dl_reuse_) {
    ++n_dl_reused_;
  } else {
    while (dl_mu_ < dogleg::kMaxMu) {
      int rc = linear_solve(1.0 / dl_mu_, &solve);
      if (rc) return rc;
      if (solve.valid) break;
      dl_mu_ *= dogleg::kMuIncreaseFactor;
    }
    if (!solve.valid) return SK_OK;  // invalid step
    dl_k_ = solve.dl;
  }
  if (!dogleg::interpolate(dl_k_, radius, &dl_a_, &dl_b_, &dl_step_norm_, model_cost_change)) return SK_OK;
  int rc = dogleg_trial(dl_a_, dl_b_, new_cost, step_norm);
  if (rc) return rc;
  *valid = std::isfinite(*step_norm);
  return SK_OK;
}

int SolverBase::step(bool* done) {
  char msg[256];
  *done = false;
  if (terminated_) { *done = true; return SK_OK; }
  // FinalizeIterationAndCheckIfMinimizerCanContinue
  if (iteration_ >= opt_.max_num_iterations) {
    sum_.termination_type = SK_NO_CONVERGENCE;
    snprintf(msg, sizeof(msg), "Maximum number of iterations reached. Number of iterations: %d.", iteration_);
    sum_.message = msg; terminated_ = true; *done = true; return SK_OK;
  }
  if (gmax_ <= opt_.gradient_tolerance) {
    sum_.termination_type = SK_CONVERGENCE;
    snprintf(msg, sizeof(msg), "Gradient tolerance reached. Gradient max norm: %e <= %e", gmax_, opt_.gradient_tolerance);
    sum_.message = msg; terminated_ = true; *done = true; return SK_OK;
  }
  if (radius_ < opt_.min_trust_region_radius) {
    sum_.termination_type = SK_CONVERGENCE;
    snprintf(msg, sizeof(msg), "Minimum trust region radius reached. Trust region radius: %e <= %e", radius_, opt_.min_trust_region_radius);
    sum_.message = msg; terminated_ = true; *done = true; return SK_OK;
  }
  const double t_iter = now();
  ++iteration_;
  ls_alpha_ = 1.0; ls_evals_ = 1; cg_iterations_last_ = 0; inner_rounds_last_ = 0;
  bool valid = false;
  double mcc = 0.0, new_cost = 0.0, step_norm = 0.0;
  int rc = try_step(radius_, &valid, &mcc, &new_cost, &step_norm);
  if (rc) return rc;
  if (valid && !(mcc > 0.0)) valid = false;
  if (!valid) {
    ++invalid_;
    if (invalid_ >= opt_.max_num_consecutive_invalid_steps) {
      sum_.termination_type = SK_FAILURE;
      snprintf(msg, sizeof(msg), "Number of consecutive invalid steps more than Solver::Options::max_num_consecutive_invalid_steps: %d",
               opt_.max_num_consecutive_invalid_steps);
      sum_.message = msg; terminated_ = true; *done = true;
      log_iteration(iteration_, 0.0, 0.0, 0.0, 0, 0, now() - t_iter);
      return SK_OK;
    }
    if (dogleg()) { dl_mu_ *= dogleg::kMuIncreaseFactor; dl_reuse_ = false; }  // DoglegStrategy::StepIsInvalid: the radius stays
    else { radius_ /= decrease_factor_; decrease_factor_ *= 2.0; }  // StepIsInvalid == StepRejected
    log_iteration(iteration_, 0.0, 0.0, 0.0, 0, 0, now() - t_iter);
    return SK_OK;
  }
  invalid_ = 0;
  bool useful = false;
  if (opt_.use_inner_iterations && inner_enabled_ && std::isfinite(new_cost)) {  // (a candidate without a cost is not refined: nothing to start from)
    const double t_inner = now(), c_tr = new_cost;
    double c_in = 0.0, norm_in = 0.0;
    bool ok = false;
    rc = refine_candidate(&c_in, &norm_in, &inner_rounds_last_, &ok);
    if (rc) return rc;
    inner_seconds_ += now() - t_inner; ++inner_steps_; inner_rounds_ += inner_rounds_last_;
    if (ok) {
      mcc += c_tr - c_in;
      useful = c_in < cost_;
      inner_enabled_ = (1.0 - c_in / c_tr) > opt_.inner_iteration_tolerance;
      new_cost = c_in; step_norm = norm_in;
    }
  }
  if (!std::isfinite(new_cost)) new_cost = std::numeric_limits<double>::max();
  const double cost_change = cost_ - new_cost;
  if (step_norm <= opt_.parameter_tolerance * (xnorm_ + opt_.parameter_tolerance)) {
    sum_.termination_type = SK_CONVERGENCE;
    snprintf(msg, sizeof(msg), "Parameter tolerance reached. Relative step_norm: %e <= %e.", step_norm / (xnorm_ + opt_.parameter_tolerance), opt_.parameter_tolerance);
    sum_.message = msg; terminated_ = true; *done = true;
    log_iteration(iteration_, cost_change, step_norm, 0.0, 1, 0, now() - t_iter);
    return SK_OK;
  }
  if (std::fabs(cost_change) <= opt_.function_tolerance * cost_) {
    sum_.termination_type = SK_CONVERGENCE;
    snprintf(msg, sizeof(msg), "Function tolerance reached. |cost_change|/cost: %e <= %e", std::fabs(cost_change) / cost_, opt_.function_tolerance);
    sum_.message = msg; terminated_ = true; *done = true;
    log_iteration(iteration_, cost_change, step_norm, 0.0, 1, 0, now() - t_iter);
    return SK_OK;
  }
  const double rho = cost_change / mcc;
  if (rho > opt_.min_relative_decrease || useful) {
    accept_candidate();
    rc = evaluate_with_jacobian(false);
    if (rc == SK_ERR_EVALUATION_FAILED) {
      sum_.termination_type = SK_FAILURE; sum_.message = "Residual and Jacobian evaluation failed.";
      terminated_ = true; *done = true; return SK_OK;
    }
    if (rc) return rc;
    if (dogleg()) {
      if (rho < dogleg::kDecreaseThreshold) radius_ *= dogleg::kRadiusDecreaseFactor;
      else if (rho > dogleg::kIncreaseThreshold) radius_ = std::min(opt_.max_trust_region_radius, std::max(radius_, dogleg::kRadiusGrowth * dl_step_norm_));
      dl_mu_ = std::max(dogleg::kMinMu, dogleg::kMuDecrease * dl_mu_ / dogleg::kMuIncreaseFactor);
      dl_reuse_ = false;
    } else {
      radius_ = radius_ / std::max(1.0 / 3.0, 1.0 - std::pow(2.0 * rho - 1.0, 3));
      radius_ = std::min(opt_.max_trust_region_radius, radius_);
      decrease_factor_ = 2.0;
    }
    ++n_success_;
    log_iteration(iteration_, cost_change, step_norm, rho, 1, 1, now() - t_iter);
  } else {
    if (dogleg()) { radius_ *= dogleg::kRadiusDecreaseFactor; dl_reuse_ = true; }
    else { radius_ /= decrease_factor_; decrease_factor_ *= 2.0; }
    ++n_unsuccess_;
    log_iteration(iteration_, cost_change, step_norm, rho, 1, 0, now() - t_iter);
  }
  return SK_OK;
}

int SolverBase::finish(Summary* s) {
  int rc = infeasible_ ? SK_OK : write_back();  // (an infeasible problem: nothing was set up, the caller's parameters stay untouched)
  if (rc) return rc;
  collect_allreduce_time(true);
  sum_.final_cost = cost_;
  sum_.num_successful_steps = n_success_;
  sum_.num_unsuccessful_steps = n_unsuccess_;
  for (int i = 0; i < 6; ++i) sum_.phase_seconds[i] = phase_[i];
  sum_.phase_seconds[6] = now();
  sum_.device_name = device_name_;
  sum_.world = opt_.world;
  sum_.linear_solver_type = opt_.linear_solver_type;
  sum_.linear_solver_type_given = opt_.linear_solver_type_given;
  sum_.use_inner_iterations = opt_.use_inner_iterations; sum_.inner_iteration_steps = inner_steps_; sum_.inner_iteration_rounds = inner_rounds_;
  sum_.inner_iterations_enabled = opt_.use_inner_iterations && inner_enabled_; sum_.inner_iteration_seconds = inner_seconds_;
  describe(&sum_);
  sum_.build_reports();
  *s = sum_;
  return SK_OK;
}

void Summary::build_reports() {
  char b[4096];
  const int iters = (int)iterations.size();
  snprintf(b, sizeof(b), "Ceres Solver Report: Iterations: %d, Initial cost: %e, Final cost: %e, Termination: %s", iters,
           initial_cost, final_cost, termination_name(termination_type));
  brief = b;
  std::string f;
  snprintf(b, sizeof(b),
           "\nSolver Summary (skeres_amd, MI355X-native Levenberg-Marquardt)\n\n"
           "Parameter blocks            % 12d\nParameters                  % 12d\nResidual blocks             % 12d\nResiduals                   % 12ld\n\n"
           "Minimizer                        TRUST_REGION\nTrust region strategy     %19s\n\n"
           "Linear solver          %22s\nDevice                 %s\nGPUs                        % 12d\n",
           num_parameter_blocks, num_parameters, num_residual_blocks, num_residuals,
           trust_region_strategy_type == SK_DOGLEG ? "DOGLEG (TRADITIONAL)" : "LEVENBERG_MARQUARDT", linear_solver_name(linear_solver_type),
           device_name.c_str(), world);
  f += b;
  if (linear_solver_type_given >= 0 && linear_solver_type_given != linear_solver_type) {
    // (Ceres reports "Given / Used"; its alternate for a Schur-type solver with nothing to eliminate is DENSE_QR too)
    snprintf(b, sizeof(b), "Linear solver given    %22s   (no 2-residual / 9- and 3-parameter block structure to eliminate: its alternate is used)\n",
             linear_solver_name(linear_solver_type_given));
    f += b;
  }
  if (linear_solver_type == SK_CGNR) {
    snprintf(b, sizeof(b), "Preconditioner         %22s\nLinear solver iterations    % 12ld\n", preconditioner_type == SK_JACOBI ? "JACOBI" : "IDENTITY", linear_solver_iterations);
    f += b;
    if (schur_elimination) {
      snprintf(b, sizeof(b), "Schur elimination      implicit: %d blocks eliminated, %d reduced columns\n", eliminated_blocks, reduced_columns);
      f += b;
    }
  }
  if (use_inner_iterations) {
    snprintf(b, sizeof(b), "Inner iterations       %d groups: %d steps refined in %ld rounds, %.6f s, %s at the end\n", inner_iteration_groups, inner_iteration_steps,
             inner_iteration_rounds, inner_iteration_seconds, inner_iterations_enabled ? "enabled" : "switched off");
    f += b;
  }
  if (linear_solver_type == SK_DENSE_SCHUR) {
    snprintf(b, sizeof(b), "Schur structure                        2,3,9\nE blocks (eliminated)       % 12d\nF blocks                    % 12d\n", num_e_blocks, num_f_blocks);
    f += b;
  }
  snprintf(b, sizeof(b),
           "\nCost:\nInitial                   % 14e\nFinal                     % 14e\nChange                    % 14e\n\n"
           "Minimizer iterations        % 12d\nSuccessful steps            % 12d\nUnsuccessful steps          % 12d\n\n"
           "Device time (s):\n  Jacobian evaluation       % 12.6f\n  Linear solver assembly    % 12.6f\n  Linear solver factor      % 12.6f\n"
           "  Back-substitution         % 12.6f\n  Cost evaluation           % 12.6f\n  All-reduce                % 12.6f\nTotal wall time             % 12.6f\n\n"
           "Termination:          %22s (%s)\n",
           initial_cost, final_cost, initial_cost - final_cost, iters, num_successful_steps, num_unsuccessful_steps, phase_seconds[0],
           phase_seconds[1], phase_seconds[2], phase_seconds[3], phase_seconds[4], phase_seconds[5], phase_seconds[6],
           termination_name(termination_type), message.c_str());
  f += b;
  full = f;
}

}  // namespace sk
