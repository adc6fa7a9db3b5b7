// Trust-region driver (host) over device linear algebra: the loop and the control flow of every strategy, written once.
// Restates the loop native Ceres [ext] runs behind `ceres.solve`
// (EX/SimpleBundleAdjuster.scala:152, EX/CurveFitting.scala:127); constants and
// update rules as published for Ceres 1.x.  Only a
// handful of scalars cross PCIe per iteration.  The trust-region strategy is
// Levenberg-Marquardt or the traditional dogleg (common.hpp: namespace dogleg).
// Parameter bounds (Problem::SetParameterLowerBound / SetParameterUpperBound): Ceres 1.x's constrained loop, restated from
// memory like the rest — x projected onto the box at iteration 0, the projected-gradient norm, the unconstrained step delta
// and its model, and a backtracking Armijo line search on cost(P(x + alpha delta)) (common.hpp: namespace bounds).  One
// deliberate departure from Ceres' defaults: the line search interpolates quadratically from function values, not cubically
// with a Jacobian at every trial point.
// Inner iterations (Solver::Options::use_inner_iterations, CGNR): a valid candidate with a positive model cost change is refined
// in place before the tolerance tests — every parameter block of an independent set minimised on its own, group after group
// (inner_plan.hpp, inner_iterations.hpp; common.hpp: namespace inner).  With c the current cost, c_tr the candidate's and c_in
// the refined candidate's: model_cost_change += c_tr - c_in, the step is successful when rho > min_relative_decrease OR
// c_in < c, the radius update takes rho as it is, and the refinement switches itself off for the rest of the solve once
// 1 - c_in / c_tr <= inner_iteration_tolerance.  A second departure from Ceres' defaults: the inner solves factor their (at most
// 16 x 16) damped normal matrices by Cholesky where Ceres runs DENSE_QR.
#pragma once
#include <chrono>
#include <memory>

#include "bal_plan.hpp"
#include "chol_kernels.hpp"
#include "common.hpp"

namespace sk {

// What the strategy kernels leave in their scalar buffers (bal_kernels.hpp: DoglegDev::scal, BoundsDev::scal; the dense kernels write
// the same layouts), as offsets into those buffers and into the pinned regions that mirror them.
enum DoglegScal {
  kDlScalars = 0,  // the eight dogleg::Scalars in the kernels' order: the observation products ...
  kDlNorms = 5,    // ... and the vector norms |g_hat|^2, g_hat . p, |p|^2
  kDlStepSq = 8,   // |x - x_new|^2 of the last combined step
  kDlScalCount
};
enum BoundsScal {
  kBdStepSq = 0,  // |x - x_new|^2 of the last candidate
  kBdGDelta,      // g . delta of the unconstrained step
  kBdMaxDelta,    // max_j |delta_j|
  kBdGradMax,     // max_j |x_j - P(x_j - g_j)|: the gradient test under bounds
  kBdXSq,         // |x|^2
  kBdActive,      // coordinates of x on a bound
  kBdScalCount
};

// What one linear solve leaves on the host (SolverBase::linear_solve); a field is set where the strategy forms it.
struct LinearSolve {
  bool valid = false;                  // the system was positive definite and the scalars are finite
  double model_cost_change = 0.0;      // of the step at this radius (LM, bounds)
  double cost = 0.0, step_norm = 0.0;  // of the candidate formed behind the back-substitution (LM, bounds)
  double g_delta = 0.0, max_delta = 0.0;  // bounds: what the line search starts from
  dogleg::Scalars dl;                  // DOGLEG
};

class SolverBase {
 public:
  SolverBase(const Options& o, Problem* p) : opt_(o), problem_(p) {}
  virtual ~SolverBase();
  int create();                 // device setup + iteration 0
  int step(bool* done);         // one trust-region iteration
  int finish(Summary* s);       // parameters back to caller memory + summary
  KernelTimer& kernel_timer() { return kt_; }
  // sk_solver_set_kernel_timing / sk_solver_kernel_seconds (a solver may keep more than one timer: one per enqueueing thread)
  virtual void set_kernel_timing(int on) { kt_.only(on == 2 ? "gemm_syrk" : ""); kt_.enable(on != 0); }
  virtual KernelTimer::Stat kernel_stat(const std::string& name) { return kt_.get_stat(name); }
  virtual double syrk_flops_per_solve() const { return 0.0; }
  virtual double syrk_c_bytes_per_solve() const { return 0.0; }  // C tiles read + written by those launches
  virtual bool stat(const std::string& name, double* value) const { (void)name; (void)value; return false; }  // sk_solver_stat
  // sk_solver_inner_iteration_blocks: per parameter block the iterations and the inner::Status of its solve in the last refinement
  virtual int inner_blocks(int* iterations, int* status) { (void)iterations; (void)status; set_error("this solver runs no inner iterations"); return SK_ERR_UNSUPPORTED; }
  bool dogleg() const { return opt_.trust_region_strategy_type == SK_DOGLEG; }
  // seconds accumulated so far in phase i (the summary's phase_seconds, readable between steps: "phase_seconds_<i>" of sk_solver_stat)
  // (between steps the stream is idle: the all-reduce phase takes in every collective's event pair first)
  double phase_seconds(int i) { if (i == 5) collect_allreduce_time(true); return (i >= 0 && i < 6) ? phase_[i] : 0.0; }
  // how a world > 1 is used (SK_DISTRIBUTION_*), with the estimates behind an automatic choice
  virtual int distribution(double* allreduce_s, double* saved_s) const {
    if (allreduce_s) *allreduce_s = 0.0;
    if (saved_s) *saved_s = 0.0;
    return SK_DISTRIBUTION_REPLICATED;
  }

 protected:
  // --- representation-specific pieces -------------------------------------
  virtual int setup() = 0;                        // build device structures, upload x
  virtual int evaluate_with_jacobian(bool first) = 0;  // at current x: cost_, gmax_, xnorm_
  // The device work of one trust-region iteration.  SolverBase::try_step owns the control flow of every strategy (Levenberg-Marquardt,
  // bounds, DOGLEG); a solver enqueues launches and reads scalars back.  linear_solve: D from the radius, the factorisation, the
  // back-substitution and what the strategy needs behind it — the candidate x + delta and its cost (LM); the candidate P(x + delta),
  // its cost, g . delta and max_j |delta_j| (bounded_); the two vectors s and g and their eight scalars, no candidate (dogleg()).
  // Every enqueued factorisation counts in n_linear_solves_.
  virtual int linear_solve(double radius, LinearSolve* out) = 0;
  // the candidate a s + b g from the vectors of the last linear solve, its cost, |x - candidate| (not finite: no step)
  virtual int dogleg_trial(double a, double b, double* cost, double* step_norm) { (void)a; (void)b; (void)cost; (void)step_norm; return SK_ERR_UNSUPPORTED; }
  // the candidate P(x + alpha delta) from the step of the last linear solve, its cost, |x - candidate|
  virtual int bounded_trial(double alpha, double* cost, double* step_norm) { (void)alpha; (void)cost; (void)step_norm; return SK_ERR_UNSUPPORTED; }
  // use_inner_iterations: the candidate of the last linear solve refined in place.  *ok: *cost is the refined candidate's cost by the
  // solver's own cost launches, *step_norm |x - refined candidate|; !*ok (the cost is not finite, or its evaluation failed): the
  // unrefined candidate is back in place.  *rounds: the lock-step rounds it took.
  virtual int refine_candidate(double* cost, double* step_norm, int* rounds, bool* ok) { (void)cost; (void)step_norm; (void)rounds; (void)ok; return SK_ERR_UNSUPPORTED; }
  bool inner_enabled_ = true;       // inner_iterations_are_enabled: once false it stays false
  int inner_steps_ = 0, inner_rounds_last_ = 0;  // iterations that were refined; the rounds of this iteration
  long inner_rounds_ = 0;
  double inner_seconds_ = 0.0;
  virtual void accept_candidate() = 0;            // x <- candidate (pointer swap)
  virtual int write_back() = 0;                   // device x -> caller memory
  virtual void describe(Summary* s) = 0;
  virtual bool supports_dogleg() const { return false; }  // linear_solve fills LinearSolve::dl, dogleg_trial is implemented
  // Parameter bounds (bounded_: the problem has a finite bound).  refuses_bounds: why this solver cannot take this problem's
  // bounds, or nullptr.
  virtual const char* refuses_bounds() const { return "parameter bounds are implemented for DENSE_SCHUR and for DENSE_QR / DENSE_NORMAL_CHOLESKY over residual blocks (not supported on dense-row problems)"; }
  int try_step(double radius, bool* valid, double* model_cost_change, double* new_cost, double* step_norm);
  int line_search(double g0, double max_delta, double* cost, double* step_norm);
  int check_bounds();  // create(): the refusals, the feasibility of the box
  bool bounded_ = false, infeasible_ = false;
  double ls_alpha_ = 1.0;          // of the last iteration
  int cg_iterations_last_ = 0;     // CGNR: CG iterations of the iteration's linear solve (the log's linear_solver_iterations)
  int ls_evals_ = 1;
  long n_ls_evals_ = 0;            // since create ("line_search_evaluations")
  long bounded_coordinates_ = 0, active_bounds_ = 0;

  int init_device();
  double now() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0_).count(); }
  void log_iteration(int it, double cost_change, double step_norm, double rho, int valid, int success, double iter_time);
  int allreduce(double* dev, size_t count);
  void add_phase(int i, hipEvent_t from, hipEvent_t to);  // phase_[i] += the time between two events that have completed
  // ... for the phases first..last of one enqueued sequence: phase i ends at ev_[i + 1] (kEvJac ... kEvCost) and begins where the one
  // before it ended, the first of them at ev_[since]
  void add_phases(int first, int last, int since = kEvBegin);
  void collect_allreduce_time(bool all);  // phase_[5] from the event pairs of collectives that have completed (all: wait for every one)
  std::vector<hipEvent_t> ar_pending_, ar_free_;

  Options opt_;
  Problem* problem_;
  hipStream_t stream_ = nullptr;
  bool own_stream_ = false;
  KernelTimer kt_;
  // phase timing (HIP events on stream_)
  enum { kEvBegin = 0, kEvJac, kEvAssemble, kEvChol, kEvBacksub, kEvCost, kEvCount };
  hipEvent_t ev_[16] = {};
  double phase_[7] = {0, 0, 0, 0, 0, 0, 0};
  // LM state
  double cost_ = 0, gmax_ = 0, xnorm_ = 0;
  double radius_ = 0, decrease_factor_ = 2.0;
  int iteration_ = 0, invalid_ = 0, n_success_ = 0, n_unsuccess_ = 0;
  bool terminated_ = false;
  // DOGLEG state (common.hpp: namespace dogleg).  dl_step_norm_: the step's norm in the diagonal-scaled space; dl_reuse_: the Jacobian
  // has not changed since the last linear solve (try_step interpolates again and solves nothing)
  double dl_mu_ = dogleg::kMinMu, dl_step_norm_ = 0.0;
  bool dl_reuse_ = false;
  long n_linear_solves_ = 0, n_dl_reused_ = 0;  // factorisations enqueued; iterations that re-interpolated (sk_solver_stat)
  dogleg::Scalars dl_k_;            // the scalars of the last linear solve
  double dl_a_ = 0.0, dl_b_ = 0.0;  // the coefficients of the last step: a s + b g
  // "bounded_coordinates", "active_bounds", "line_search_evaluations";
  // "inner_iteration_steps", "inner_iteration_rounds", "inner_iterations_enabled", "inner_iteration_seconds";
  // "linear_solves", "dogleg_reused_steps", "dogleg_mu"; under DOGLEG also dl_k_, dl_a_, dl_b_ as "dogleg_w_r", ..., "dogleg_b"
  bool strategy_stat(const std::string& name, double* value) const;
  Summary sum_;
  std::chrono::steady_clock::time_point t0_;
  std::string device_name_;
};

// BAL-shaped problems (2 residuals, one 9-block + one 3-block per residual
// block): Schur elimination of the 3-blocks + dense Cholesky of the reduced system.
std::unique_ptr<SolverBase> make_bal_solver(const Options& o, Problem* p);
// (the host planning of that path, and the plans as tests and tools read them: bal_plan.hpp)
// Generic dense Jacobian path: DENSE_QR / DENSE_NORMAL_CHOLESKY.
std::unique_ptr<SolverBase> make_dense_solver(const Options& o, Problem* p);
// Tall dense rows over one parameter block (transposed Jacobian + long-K MFMA SYRK): DENSE_NORMAL_CHOLESKY.
std::unique_ptr<SolverBase> make_dense_rows_solver(const Options& o, Problem* p);
bool problem_is_dense_rows(const Problem& p);
// Block-sparse Jacobian, never J^T J: CGNR (preconditioned conjugate gradients on the damped normal equations as two products).
std::unique_ptr<SolverBase> make_cgnr_solver(const Options& o, Problem* p);

}  // namespace sk
