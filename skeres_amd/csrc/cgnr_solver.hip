// CGNR: Levenberg-Marquardt whose step is an inexact Newton step — preconditioned conjugate gradients on the damped normal
// equations (J^T J + D^2) y = -J^T r, the matrix applied as two products with the block-sparse Jacobian and never formed
// (common.hpp: namespace cgnr; Ceres 1.x's ConjugateGradientsSolver, restated from memory).  The Jacobian is Problem::Evaluate's
// values array (evaluate_plan.hpp, evaluate_kernels.hip) over every residual block, scaled in place by the Jacobi scaling; the
// plan of the products and of the block-Jacobi preconditioner: cgnr_plan.hpp; the kernels: cgnr_kernels.hip.
//
// The batch protocol.  The scalars of the CG loop and its iteration counter, done flag and status live on the device (CgnrScal,
// CgnrFlag); a scalar kernel per iteration decides whether the loop goes on, and every kernel of the loop returns at once when
// the flag is set.  The host enqueues cgnr::kBatch iterations, reads the flags back, and stops enqueueing when the loop is done:
// ordinary stream-ordered launches, no kernel waits for another, no graph.  What is enqueued past the end does nothing, so the
// step is the same bytes for every batch size.
//
// Schur elimination (sk_options_set_schur_elimination; the plan: cgnr_plan.hpp).  With H = J^T J + D^2 = [[U, W], [W^T, V]] over
// the kept blocks F and an independent set E of eliminated blocks (V block diagonal), the same loop solves S y_F = s with
// S = U - W V^-1 W^T and s = b_F - W V^-1 b_E, then y_E = V^-1 (b_E - W^T y_F); model cost change, candidate and cost come from
// the full step as without it.  S is never formed: S v = J_F^T P (J_F v) + D_F^2 v with P = I - J_E V^-1 J_E^T, so an
// application is the two products over F's index arrays with one projection launch (cgnr_eliminate_kernel) between them.
// JACOBI is then the block diagonal of S (cgnr_schur_diag_kernel), formed once per linear solve because the radius changes V.
// The vectors keep the full tangent space's columns; the entries of E stay zero until the back-substitution.  Without the option
// the launches are the ones above, unchanged.
//
// Inner iterations (sk_options_set_use_inner_iterations; inner_iterations.hpp).  The component is handed this solver's device
// Jacobian, values array, staging and residual and cost-term arrays, and refines the candidate x_new_ in place.  Its rounds read and
// leave the values UNSCALED, at points other than x.  So nothing of a refinement is copied: when the refined step is rejected, the
// next linear solve begins with the evaluation launches at x again (values, residuals, cost terms) and the scaling in place —
// the same launches on the same point, hence the same bytes as before; an accepted step evaluates at the new point anyway.  The
// sums, the gradient and the scalars of x are not touched by a refinement (it has buffers of its own for a block's g and H).
#include <algorithm>
#include <cmath>
#include <limits>

#include "cgnr_kernels.hpp"
#include "cgnr_plan.hpp"
#include "evaluate_kernels.hpp"
#include "inner_iterations.hpp"
#include "jacobian_device.hpp"
#include "solver.hpp"

namespace sk {
namespace {

static_assert(kCgnrPartSlots == cgnr::kPartSlots, "jacobian_plan.hpp restates common.hpp's constant for the host-only plans");
static_assert(kCgnrMaxBlock == kParamMaxSize, "a block's Plus and its Cholesky live in one lane");

class CgnrSolver : public SolverBase {
 public:
  CgnrSolver(const Options& o, Problem* p) : SolverBase(o, p) {}
  ~CgnrSolver() override { if (h_scal_) (void)hipHostFree(h_scal_); if (h_flags_) (void)hipHostFree(h_flags_); }

 protected:
  int setup() override;
  int evaluate_with_jacobian(bool first) override;
  int linear_solve(double radius, LinearSolve* out) override;
  const char* refuses_bounds() const override { return "parameter bounds under CGNR are not supported (DENSE_SCHUR and DENSE_QR / DENSE_NORMAL_CHOLESKY take them)"; }
  void accept_candidate() override { std::swap(x_, x_new_); }
  int refine_candidate(double* cost, double* step_norm, int* rounds, bool* ok) override;
  int write_back() override;
  void describe(Summary* s) override {
    s->num_parameter_blocks = (int)problem_->block_size.size();
    s->num_parameters = plan_.cols.num_ambient; s->num_residual_blocks = (int)problem_->rb_functor.size(); s->num_residuals = plan_.eval.num_rows;
    s->preconditioner_type = opt_.preconditioner_type; s->linear_solver_iterations = n_cg_iterations_;
    s->schur_elimination = schur(); s->eliminated_blocks = (int)plan_.E.cb.size(); s->reduced_columns = plan_.reduced_cols;
    s->inner_iteration_groups = (int)inner_plan_.groups.size();
  }
  int inner_blocks(int* iterations, int* status) override {
    if (!opt_.use_inner_iterations) { set_error("use_inner_iterations is off"); return SK_ERR_INVALID_ARGUMENT; }
    return inner_.blocks(iterations, status);
  }
  bool stat(const std::string& name, double* value) const override {
    if (name == "cg_iterations") { *value = (double)n_cg_iterations_; return true; }
    if (name == "cg_iterations_last") { *value = (double)cg_iterations_last_solve_; return true; }
    if (name == "cg_status_last") { *value = (double)cg_status_last_; return true; }
    if (name == "cg_batches") { *value = (double)n_batches_; return true; }
    if (name == "jacobian_nonzeros") { *value = (double)plan_.eval.num_nonzeros; return true; }
    if (name == "inner_iteration_groups") { *value = (double)inner_plan_.groups.size(); return true; }
    if (name == "graph_replay") { *value = 0.0; return true; }
    if (name == "schur_elimination") { *value = schur() ? 1.0 : 0.0; return true; }
    if (name == "eliminated_blocks") { *value = (double)plan_.E.cb.size(); return true; }
    if (name == "reduced_columns") { *value = (double)(schur() ? plan_.reduced_cols : n_); return true; }
    if (name == "schur_diagonal_pairs") { *value = (double)plan_.fp_e.size(); return true; }
    if (name == "tape_blocks") {
      size_t c = 0;
      for (const EvaluateGroup& G : plan_.eval.groups) if (G.functor >= kTapeFunctorBase) c += G.members.size();
      *value = (double)c;
      return true;
    }
    return strategy_stat(name, value);
  }

 private:
  int evaluate(const double* x_dev, bool jac);
  void finish(const double* x_dev, bool jac);
  int enqueue_cg_iteration(int it);
  bool jacobi() const { return opt_.preconditioner_type == SK_JACOBI; }
  bool schur() const { return opt_.cgnr_schur_elimination; }
  int setup_schur();
  int upload_subset(const CgnrColumnSubset& S, DevBuf<int>* bufs, CgnrCols* cols);
  void project(double* w, const int* flags) {  // w <- w - J_E V^-1 J_E^T w
    launch_cgnr_eliminate(kCgnrElimProject, jac_, cols_e_, b_e_long_slots_.p, b_L_.p, nullptr, w, nullptr, b_e_part_.p, flags, stream_);
  }

  CgnrPlan plan_;
  InnerPlan inner_plan_;
  InnerIterations inner_;
  DevBuf<double> b_x_unrefined_;
  bool values_stale_ = false;  // a refinement has overwritten values, residuals and cost terms of x: evaluate again before they are read
  int restore_jacobian();
  int n_ = 0, ng_ = 0, m_ = 0, nb_ = 0, num_pb_ = 0, update_parts_ = 0;
  DeviceJacobian dj_;  // the problem and the evaluation's plan on the device (uploaded once); its x is the starting point
  // the solver's plan on the device
  DevBuf<size_t> b_blk_stage_cost_;
  DevBuf<int> b_slot_col_, b_slot_size_, b_row_block_, b_cb_col_, b_cb_size_, b_cb_moff_, b_cb_slots_, b_part_cb_, b_part_begin_, b_part_end_, b_part_out_,
      b_long_cb_, b_long_begin_, b_flags_;
  // the state: the candidate; residuals and cost terms at x and at the candidate; the vectors of the tangent space
  DevBuf<double> b_xb_, b_r_, b_rc_, b_cterm_, b_cterm_c_, b_scale_, b_gs_, b_b_, b_D2_, b_bsum_, b_L_, b_y_, b_res_, b_z_, b_p_, b_q_, b_w_,
      b_part_, b_jtw_part_, b_bd_part_, b_scal_;
  CgnrJac jac_{};
  CgnrCols cols_{};
  // the Schur elimination: F's and E's index arrays (kSubsetBufs each), the pairs; s, the sums of S's diagonal and the partial sums.
  // Without it cg_jac_ and cg_cols_ are jac_ and cols_, and b_rhs_ is b.
  static constexpr int kSubsetBufs = 10;
  DevBuf<int> b_f_[kSubsetBufs], b_e_[kSubsetBufs], b_slot_size_f_, b_e_long_slots_, b_fp_part_f_, b_fp_part_begin_, b_fp_part_end_, b_fp_part_out_, b_fp_long_f_,
      b_fp_long_begin_, b_fp_e_, b_fp_slot_begin_, b_fp_slot_g_, b_fp_slot_e_;
  DevBuf<double> b_s_, b_sdiag_, b_e_part_, b_sd_part_;
  CgnrJac cg_jac_{};
  CgnrCols cg_cols_{}, cols_e_{};
  CgnrPairs pairs_{};
  const double* b_rhs_ = nullptr;
  int cg_update_parts_ = 0;
  double* x_ = nullptr; double* x_new_ = nullptr;
  double* h_scal_ = nullptr;
  int* h_flags_ = nullptr;  // [kCgFlagCount] the CG flags, then the evaluation's failure flag
  long n_cg_iterations_ = 0, n_batches_ = 0;
  int cg_iterations_last_solve_ = 0, cg_status_last_ = cgnr::kRunning;
};

int CgnrSolver::setup() {
  const Problem& p = *problem_;
  {
    const std::string refusal = cgnr_refusal(p, opt_.world, dogleg());
    if (!refusal.empty()) { set_error("%s", refusal.c_str()); return SK_ERR_UNSUPPORTED; }
  }
  if (p.rb_functor.empty()) { set_error("problem has no residual blocks"); return SK_ERR_INVALID_ARGUMENT; }
  std::string why;
  int rc = cgnr_plan_build(p, &plan_, &why, schur());
  if (rc != SK_OK) { set_error("%s", why.c_str()); return rc; }
  if (opt_.use_inner_iterations) {
    rc = inner_plan_build(p, plan_, opt_.inner_ordering_blocks, opt_.inner_ordering_groups, &inner_plan_, &why);
    if (rc != SK_OK) { set_error("%s", why.c_str()); return rc; }
  }
  const EvaluatePlan& E = plan_.eval;
  const TangentColumns& T = plan_.cols;
  const PartList& L = plan_.parts;
  n_ = T.num_cols; ng_ = T.num_ambient; m_ = E.num_rows; nb_ = (int)E.blocks.size(); num_pb_ = (int)p.block_ptr.size();
  if (n_ == 0) { set_error("every parameter block is constant: nothing to optimise"); return SK_ERR_INVALID_ARGUMENT; }
  hipStream_t s = stream_;

  // the evaluation's side; a recorded functor's tape goes to the device once
  for (const EvaluateGroup& G : E.groups) {
    if (G.functor < kTapeFunctorBase) continue;
    const Tape& t = *p.tapes[G.functor - kTapeFunctorBase];
    if (tape_pick_width(t, 128) == 0 || tape_lds_bytes(t, 0, 128) > kTapeLdsBudget) {
      set_error("a recorded functor needs %d registers: more than the device interpreter holds", t.num_registers);
      return SK_ERR_UNSUPPORTED;
    }
  }
  dj_.gather(p, E, param_blocks(p, E, &T), /*apply_loss*/ true);
  rc = dj_.upload(/*want_values*/ true, /*by_column*/ true, s);
  if (rc == SK_OK) rc = dj_.upload_tapes();
  if (rc != SK_OK) return rc;
  SK_HIP_TRY(b_xb_.alloc((size_t)ng_));
  x_ = dj_.x(); x_new_ = b_xb_.p;
  SK_HIP_TRY(b_r_.alloc((size_t)m_)); SK_HIP_TRY(b_rc_.alloc((size_t)m_)); SK_HIP_TRY(b_cterm_.alloc((size_t)nb_)); SK_HIP_TRY(b_cterm_c_.alloc((size_t)nb_));

  // the solver's side
  SK_HIP_TRY(b_blk_stage_cost_.upload(plan_.blk_stage_cost, s));
  SK_HIP_TRY(upload_padded(b_slot_col_, plan_.slot_col, s)); SK_HIP_TRY(upload_padded(b_slot_size_, plan_.slot_size, s));
  SK_HIP_TRY(b_row_block_.upload(plan_.row_block, s));
  SK_HIP_TRY(b_cb_col_.upload(T.cb_col, s)); SK_HIP_TRY(b_cb_size_.upload(T.cb_size, s)); SK_HIP_TRY(b_cb_moff_.upload(plan_.cb_moff, s));
  SK_HIP_TRY(upload_padded(b_cb_slots_, plan_.cb_slots, s));
  SK_HIP_TRY(b_part_cb_.upload(L.owner, s)); SK_HIP_TRY(b_part_begin_.upload(L.begin, s)); SK_HIP_TRY(b_part_end_.upload(L.end, s));
  SK_HIP_TRY(b_part_out_.upload(L.out, s));
  SK_HIP_TRY(upload_padded(b_long_cb_, L.long_owner, s)); SK_HIP_TRY(b_long_begin_.upload(L.long_begin, s));
  const size_t msize = (size_t)plan_.cb_moff.back();
  for (DevBuf<double>* v : {&b_scale_, &b_gs_, &b_b_, &b_D2_, &b_y_, &b_res_, &b_z_, &b_p_, &b_q_}) SK_HIP_TRY(v->alloc((size_t)n_));
  SK_HIP_TRY(b_bsum_.alloc(msize)); SK_HIP_TRY(b_L_.alloc(msize)); SK_HIP_TRY(b_w_.alloc((size_t)m_));
  { std::vector<double> ones((size_t)n_, 1.0); SK_HIP_TRY(hipMemcpyAsync(b_scale_.p, ones.data(), ones.size() * sizeof(double), hipMemcpyHostToDevice, s)); SK_HIP_TRY(hipStreamSynchronize(s)); }
  const int ncb = (int)T.cb_col.size();
  update_parts_ = (ncb + kCgnrBlockChunk - 1) / kCgnrBlockChunk;
  const size_t parts = std::max({(size_t)3 * update_parts_, (size_t)(n_ / kCgnrDotChunk + 1), (size_t)(m_ / kCgnrDotChunk + 1), (size_t)(num_pb_ / 256 + 1),
                                 (size_t)(nb_ / kEvaluateSumChunk + 1), (size_t)(ng_ / kCgnrDotChunk + 1)});
  SK_HIP_TRY(b_part_.alloc(parts));
  SK_HIP_TRY(b_jtw_part_.alloc(std::max<size_t>((size_t)L.num_partials * kCgnrLanes, 1)));
  SK_HIP_TRY(b_bd_part_.alloc(std::max<size_t>((size_t)L.num_partials * 256, 1)));
  SK_HIP_TRY(b_scal_.alloc(kCgScalCount)); SK_HIP_TRY(b_scal_.zero(s));
  SK_HIP_TRY(b_flags_.alloc(kCgFlagCount)); SK_HIP_TRY(b_flags_.zero(s));
  SK_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_scal_), kCgScalCount * sizeof(double), hipHostMallocDefault));
  SK_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_flags_), (kCgFlagCount + 1) * sizeof(int), hipHostMallocDefault));

  jac_.num_rows = m_; jac_.row_block = b_row_block_.p; jac_.row_off = dj_.row_off(); jac_.val_off = dj_.val_off(); jac_.slot_begin = dj_.slot_begin();
  jac_.slot_pos = dj_.slot_pos(); jac_.slot_col = b_slot_col_.p; jac_.slot_size = b_slot_size_.p; jac_.slot_owner = dj_.slot_owner(); jac_.values = dj_.values();
  cols_.num_cb = ncb; cols_.num_parts = (int)L.owner.size(); cols_.num_long = (int)L.long_owner.size();
  cols_.cb_col = b_cb_col_.p; cols_.cb_size = b_cb_size_.p; cols_.cb_moff = b_cb_moff_.p; cols_.cb_slots = b_cb_slots_.p;
  cols_.part_cb = b_part_cb_.p; cols_.part_begin = b_part_begin_.p; cols_.part_end = b_part_end_.p; cols_.part_out = b_part_out_.p;
  cols_.long_cb = b_long_cb_.p; cols_.long_begin = b_long_begin_.p;
  cg_jac_ = jac_; cg_cols_ = cols_; b_rhs_ = b_b_.p; cg_update_parts_ = update_parts_;
  if (schur()) { rc = setup_schur(); if (rc != SK_OK) return rc; }
  if (opt_.use_inner_iterations) {
    InnerIterations::Shared sh;
    sh.dj = &dj_; sh.jac = jac_; sh.group_stage_cost = &plan_.group_stage_cost; sh.blk_stage_cost = b_blk_stage_cost_.p;
    sh.r = b_r_.p; sh.rc = b_rc_.p; sh.cterm = b_cterm_.p; sh.cterm_c = b_cterm_c_.p; sh.jtw_partial = b_jtw_part_.p; sh.bd_partial = b_bd_part_.p;
    sh.num_cols = n_; sh.num_ambient = ng_; sh.num_pb = num_pb_; sh.matrix_entries = msize;
    rc = inner_.setup(inner_plan_, sh, s);
    if (rc != SK_OK) return rc;
    SK_HIP_TRY(b_x_unrefined_.alloc((size_t)ng_));
  }
  SK_HIP_TRY(hipStreamSynchronize(s));
  return SK_OK;
}

int CgnrSolver::upload_subset(const CgnrColumnSubset& S, DevBuf<int>* b, CgnrCols* cols) {
  hipStream_t s = stream_;
  const PartList& L = S.parts;
  SK_HIP_TRY(upload_padded(b[0], S.cb_col, s)); SK_HIP_TRY(upload_padded(b[1], S.cb_size, s)); SK_HIP_TRY(upload_padded(b[2], S.cb_moff, s));
  SK_HIP_TRY(upload_padded(b[3], S.cb_slots, s));
  SK_HIP_TRY(upload_padded(b[4], L.owner, s)); SK_HIP_TRY(upload_padded(b[5], L.begin, s)); SK_HIP_TRY(upload_padded(b[6], L.end, s)); SK_HIP_TRY(upload_padded(b[7], L.out, s));
  SK_HIP_TRY(upload_padded(b[8], L.long_owner, s)); SK_HIP_TRY(b[9].upload(L.long_begin, s));
  cols->num_cb = (int)S.cb.size(); cols->num_parts = (int)L.owner.size(); cols->num_long = (int)L.long_owner.size();
  cols->cb_col = b[0].p; cols->cb_size = b[1].p; cols->cb_moff = b[2].p; cols->cb_slots = b[3].p;
  cols->part_cb = b[4].p; cols->part_begin = b[5].p; cols->part_end = b[6].p; cols->part_out = b[7].p;
  cols->long_cb = b[8].p; cols->long_begin = b[9].p;
  return SK_OK;
}

// The index arrays of F, E and the pairs; the loop then runs on F's (cg_jac_, cg_cols_) with s as its right-hand side.
int CgnrSolver::setup_schur() {
  hipStream_t s = stream_;
  int rc = upload_subset(plan_.F, b_f_, &cg_cols_);
  if (rc == SK_OK) rc = upload_subset(plan_.E, b_e_, &cols_e_);
  if (rc != SK_OK) return rc;
  SK_HIP_TRY(upload_padded(b_slot_size_f_, plan_.slot_size_f, s));
  cg_jac_.slot_size = b_slot_size_f_.p;
  std::vector<int> long_slots;
  for (int e : plan_.E.parts.long_owner) { long_slots.push_back(plan_.E.cb_begin[e]); long_slots.push_back(plan_.E.cb_begin[e + 1]); }
  SK_HIP_TRY(upload_padded(b_e_long_slots_, long_slots, s));
  const PartList& L = plan_.fp_parts;
  SK_HIP_TRY(upload_padded(b_fp_part_f_, L.owner, s)); SK_HIP_TRY(upload_padded(b_fp_part_begin_, L.begin, s)); SK_HIP_TRY(upload_padded(b_fp_part_end_, L.end, s));
  SK_HIP_TRY(upload_padded(b_fp_part_out_, L.out, s)); SK_HIP_TRY(upload_padded(b_fp_long_f_, L.long_owner, s)); SK_HIP_TRY(b_fp_long_begin_.upload(L.long_begin, s));
  SK_HIP_TRY(upload_padded(b_fp_e_, plan_.fp_e, s)); SK_HIP_TRY(b_fp_slot_begin_.upload(plan_.fp_slot_begin, s));
  SK_HIP_TRY(upload_padded(b_fp_slot_g_, plan_.fp_slot_g, s)); SK_HIP_TRY(upload_padded(b_fp_slot_e_, plan_.fp_slot_e, s));
  pairs_.num_parts = (int)L.owner.size(); pairs_.num_long = (int)L.long_owner.size();
  pairs_.part_f = b_fp_part_f_.p; pairs_.part_begin = b_fp_part_begin_.p; pairs_.part_end = b_fp_part_end_.p; pairs_.part_out = b_fp_part_out_.p;
  pairs_.long_f = b_fp_long_f_.p; pairs_.long_begin = b_fp_long_begin_.p;
  pairs_.pair_e = b_fp_e_.p; pairs_.cb_size = b_cb_size_.p; pairs_.cb_moff = b_cb_moff_.p;
  pairs_.pair_slot_begin = b_fp_slot_begin_.p; pairs_.slot_g = b_fp_slot_g_.p; pairs_.slot_e = b_fp_slot_e_.p;
  SK_HIP_TRY(b_s_.alloc((size_t)n_)); SK_HIP_TRY(b_s_.zero(s));
  SK_HIP_TRY(b_q_.zero(s));  // (the entries of E are never written and are read by the dot product p . q)
  SK_HIP_TRY(b_sdiag_.alloc((size_t)plan_.cb_moff.back()));
  SK_HIP_TRY(b_e_part_.alloc(std::max<size_t>((size_t)plan_.E.parts.num_partials * kCgnrLanes, 1)));
  SK_HIP_TRY(b_sd_part_.alloc(std::max<size_t>((size_t)L.num_partials * 256, 1)));
  b_rhs_ = b_s_.p;
  cg_update_parts_ = ((int)plan_.F.cb.size() + kCgnrBlockChunk - 1) / kCgnrBlockChunk;
  return SK_OK;
}

// The evaluation launches of one point, with the Jacobian planes (jac) or into the residual-only staging.
int CgnrSolver::evaluate(const double* x_dev, bool jac) { return dj_.evaluate(x_dev, jac, jac ? nullptr : &plan_.group_stage_cost); }

// Loss correction, projection into the tangent space and the scatter into the values array (jac), or residuals and cost terms alone.
void CgnrSolver::finish(const double* x_dev, bool jac) {
  if (jac) dj_.finish(x_dev, b_r_.p, dj_.values(), b_cterm_.p);
  else dj_.finish(x_dev, b_rc_.p, nullptr, b_cterm_c_.p, b_blk_stage_cost_.p);
}

// After a refinement whose step was rejected: values, residuals and cost terms of x again, as evaluate_with_jacobian left them.
int CgnrSolver::restore_jacobian() {
  int rc = evaluate(x_, true);
  if (rc) return rc;
  finish(x_, true);
  if (opt_.jacobi_scaling) launch_cgnr_scale_apply(jac_, b_scale_.p, stream_);
  values_stale_ = false;
  return SK_OK;
}

// The candidate x_new_ refined in place, its cost by the cost launches of linear_solve, |x - x_new_|.
int CgnrSolver::refine_candidate(double* cost, double* step_norm, int* rounds, bool* ok) {
  hipStream_t s = stream_;
  *ok = false;
  SK_HIP_TRY(hipMemcpyAsync(b_x_unrefined_.p, x_new_, (size_t)ng_ * sizeof(double), hipMemcpyDeviceToDevice, s));
  values_stale_ = true;
  int rc = inner_.refine(x_new_, rounds);
  if (rc) return rc;
  SK_HIP_TRY(hipMemsetAsync(dj_.fail_flag(), 0, sizeof(int), s));
  rc = evaluate(x_new_, false);
  if (rc) return rc;
  finish(x_new_, false);
  launch_evaluate_cost(b_cterm_c_.p, nb_, b_part_.p, b_scal_.p + kCgCandCost, s);
  launch_inner_diff_sq(x_, x_new_, ng_, b_part_.p, s);
  launch_cgnr_sum(b_part_.p, (ng_ + kCgnrDotChunk - 1) / kCgnrDotChunk, b_scal_.p + kCgStepSq, nullptr, s);
  SK_HIP_TRY(hipMemcpyAsync(h_scal_, b_scal_.p, kCgScalCount * sizeof(double), hipMemcpyDeviceToHost, s));
  SK_HIP_TRY(hipMemcpyAsync(h_flags_ + kCgFlagCount, dj_.fail_flag(), sizeof(int), hipMemcpyDeviceToHost, s));
  SK_HIP_TRY(hipStreamSynchronize(s));
  SK_HIP_TRY(hipGetLastError());
  if (h_flags_[kCgFlagCount] || !std::isfinite(h_scal_[kCgCandCost]) || !std::isfinite(h_scal_[kCgStepSq])) {
    SK_HIP_TRY(hipMemcpyAsync(x_new_, b_x_unrefined_.p, (size_t)ng_ * sizeof(double), hipMemcpyDeviceToDevice, s));
    SK_HIP_TRY(hipStreamSynchronize(s));
    return SK_OK;
  }
  *ok = true; *cost = h_scal_[kCgCandCost]; *step_norm = std::sqrt(h_scal_[kCgStepSq]);
  return SK_OK;
}

int CgnrSolver::evaluate_with_jacobian(bool first) {
  hipStream_t s = stream_;
  values_stale_ = false;
  SK_HIP_TRY(hipEventRecord(ev_[kEvBegin], s));
  SK_HIP_TRY(hipMemsetAsync(dj_.fail_flag(), 0, sizeof(int), s));
  int rc = evaluate(x_, true);
  if (rc) return rc;
  finish(x_, true);
  if (opt_.jacobi_scaling) {
    if (first) {  // column scales from the sums of the unscaled Jacobian, held for the whole solve
      launch_cgnr_block_diag(jac_, cols_, b_bsum_.p, b_bd_part_.p, s);
      launch_cgnr_scale_compute(cols_, b_bsum_.p, b_scale_.p, s);
    }
    launch_cgnr_scale_apply(jac_, b_scale_.p, s);
  }
  launch_cgnr_jtw(kCgnrJtwPlain, jac_, cols_, b_r_.p, nullptr, nullptr, nullptr, nullptr, b_gs_.p, b_jtw_part_.p, nullptr, s);
  launch_cgnr_gradient_norms(b_gs_.p, b_scale_.p, n_, x_, ng_, b_b_.p, b_scal_.p, s);
  launch_evaluate_cost(b_cterm_.p, nb_, b_part_.p, b_scal_.p + kCgCost, s);
  SK_HIP_TRY(hipEventRecord(ev_[kEvJac], s));
  launch_cgnr_block_diag(jac_, cols_, b_bsum_.p, b_bd_part_.p, s);  // of the scaled Jacobian: what every linear solve at this point starts from
  SK_HIP_TRY(hipEventRecord(ev_[kEvAssemble], s));
  SK_HIP_TRY(hipMemcpyAsync(h_scal_, b_scal_.p, kCgScalCount * sizeof(double), hipMemcpyDeviceToHost, s));
  SK_HIP_TRY(hipMemcpyAsync(h_flags_ + kCgFlagCount, dj_.fail_flag(), sizeof(int), hipMemcpyDeviceToHost, s));
  SK_HIP_TRY(hipStreamSynchronize(s));
  SK_HIP_TRY(hipGetLastError());
  add_phases(0, 1);
  cost_ = h_scal_[kCgCost]; gmax_ = h_scal_[kCgGradMax]; xnorm_ = std::sqrt(h_scal_[kCgXSq]);
  if (h_flags_[kCgFlagCount] || !std::isfinite(cost_) || !std::isfinite(gmax_)) return SK_ERR_EVALUATION_FAILED;
  return SK_OK;
}

// Iteration `it` of the loop of common.hpp's namespace cgnr.  At its start z = M^-1 res, rho = res . z and beta are in place
// (the fused update and the scalar kernel that ended the iteration before, or that began the solve).
int CgnrSolver::enqueue_cg_iteration(int it) {
  hipStream_t s = stream_;
  const int* flags = b_flags_.p;
  const double* L = jacobi() ? b_L_.p : nullptr;
  launch_cgnr_jp(cg_jac_, b_z_.p, b_p_.p, b_scal_.p, b_w_.p, flags, s);                                                      // w = J p, p = z + beta p
  if (schur()) project(b_w_.p, flags);
  launch_cgnr_jtw(kCgnrJtwCg, cg_jac_, cg_cols_, b_w_.p, b_D2_.p, b_z_.p, b_p_.p, b_scal_.p, b_q_.p, b_jtw_part_.p, flags, s);   // q = J^T w + D2 p; p stored
  launch_cgnr_dot(0, b_p_.p, b_q_.p, n_, b_part_.p, flags, s);
  launch_cgnr_scalar_alpha(b_part_.p, (n_ + kCgnrDotChunk - 1) / kCgnrDotChunk, b_scal_.p, b_flags_.p, s);                // alpha = rho / p . q
  if (it % cgnr::kResidualResetPeriod == 0) {  // res = b - A x
    launch_cgnr_axpy(b_scal_.p, b_p_.p, b_y_.p, n_, flags, s);
    launch_cgnr_jp(cg_jac_, b_y_.p, nullptr, nullptr, b_w_.p, flags, s);
    if (schur()) project(b_w_.p, flags);
    launch_cgnr_jtw(kCgnrJtwVector, cg_jac_, cg_cols_, b_w_.p, b_D2_.p, b_y_.p, nullptr, nullptr, b_q_.p, b_jtw_part_.p, flags, s);
    launch_cgnr_update(kCgnrReset, cg_cols_, L, b_rhs_, b_p_.p, b_q_.p, b_scal_.p, b_y_.p, b_res_.p, b_z_.p, b_part_.p, flags, s);
  } else {     // x += alpha p, res -= alpha q
    launch_cgnr_update(kCgnrStep, cg_cols_, L, b_rhs_, b_p_.p, b_q_.p, b_scal_.p, b_y_.p, b_res_.p, b_z_.p, b_part_.p, flags, s);
  }
  launch_cgnr_scalar_end(b_part_.p, cg_update_parts_, opt_.eta, opt_.min_linear_solver_iterations, opt_.max_linear_solver_iterations, b_scal_.p, b_flags_.p, s);
  return SK_OK;
}

int CgnrSolver::linear_solve(double radius, LinearSolve* out) {
  hipStream_t s = stream_;
  *out = LinearSolve();
  ++n_linear_solves_;
  const int max_it = opt_.max_linear_solver_iterations;
  const int batch = dev_knobs().cgnr_batch > 0 ? dev_knobs().cgnr_batch : cgnr::kBatch;
  if (values_stale_) { const int rc = restore_jacobian(); if (rc) return rc; }
  SK_HIP_TRY(hipEventRecord(ev_[kEvBegin], s));
  SK_HIP_TRY(hipMemsetAsync(b_flags_.p, 0, kCgFlagCount * sizeof(int), s));
  launch_cgnr_precond_factor(cols_, b_bsum_.p, opt_.min_lm_diagonal, opt_.max_lm_diagonal, radius, b_D2_.p, jacobi() || schur() ? b_L_.p : nullptr, b_flags_.p, s);
  if (schur()) {  // V's factors are in place: the block diagonal of S over F's (JACOBI), s = -J_F^T P r
    if (jacobi()) {
      launch_cgnr_schur_diag(jac_, cg_cols_, pairs_, b_L_.p, b_sdiag_.p, b_sd_part_.p, s);
      launch_cgnr_precond_factor(cg_cols_, b_bsum_.p, opt_.min_lm_diagonal, opt_.max_lm_diagonal, radius, b_D2_.p, b_L_.p, b_flags_.p, s, b_sdiag_.p);
    }
    SK_HIP_TRY(hipMemcpyAsync(b_w_.p, b_r_.p, (size_t)m_ * sizeof(double), hipMemcpyDeviceToDevice, s));
    project(b_w_.p, nullptr);
    launch_cgnr_jtw(kCgnrJtwNegated, jac_, cg_cols_, b_w_.p, nullptr, nullptr, nullptr, nullptr, b_s_.p, b_jtw_part_.p, nullptr, s);
  }
  SK_HIP_TRY(hipEventRecord(ev_[kEvAssemble], s));

  // x = 0, res = b, z = M^-1 res, rho; then iterations in batches until the device says done
  SK_HIP_TRY(hipMemsetAsync(b_y_.p, 0, (size_t)n_ * sizeof(double), s));
  SK_HIP_TRY(hipMemsetAsync(b_p_.p, 0, (size_t)n_ * sizeof(double), s));
  launch_cgnr_update(kCgnrInit, cg_cols_, jacobi() ? b_L_.p : nullptr, b_rhs_, b_p_.p, b_q_.p, b_scal_.p, b_y_.p, b_res_.p, b_z_.p, b_part_.p, nullptr, s);
  launch_cgnr_scalar_init(b_part_.p, cg_update_parts_, b_scal_.p, b_flags_.p, s);
  int enqueued = 0;
  const bool no_loop = schur() && plan_.F.cb.empty();  // every moving block is independent of the others: the back-substitution is the solve
  if (no_loop) {
    SK_HIP_TRY(hipMemcpyAsync(h_flags_, b_flags_.p, kCgFlagCount * sizeof(int), hipMemcpyDeviceToHost, s));
    SK_HIP_TRY(hipStreamSynchronize(s));
    h_flags_[kCgIt] = 0; h_flags_[kCgDone] = 1; h_flags_[kCgStatus] = cgnr::kConverged;
  }
  while (!no_loop) {
    for (int k = 0; k < batch && enqueued < max_it; ++k) { int rc = enqueue_cg_iteration(++enqueued); if (rc) return rc; }
    SK_HIP_TRY(hipMemcpyAsync(h_flags_, b_flags_.p, kCgFlagCount * sizeof(int), hipMemcpyDeviceToHost, s));
    SK_HIP_TRY(hipStreamSynchronize(s));
    ++n_batches_;
    if (h_flags_[kCgDone] || h_flags_[kCgFail] || enqueued >= max_it) break;
  }
  SK_HIP_TRY(hipGetLastError());
  SK_HIP_TRY(hipEventRecord(ev_[kEvChol], s));
  cg_iterations_last_solve_ = cg_iterations_last_ = h_flags_[kCgIt];
  n_cg_iterations_ += h_flags_[kCgIt];
  cg_status_last_ = h_flags_[kCgDone] ? h_flags_[kCgStatus] : (int)cgnr::kIterationLimit;  // (a limit of 0 iterations: nothing ran)
  if (h_flags_[kCgFail] || cg_status_last_ == cgnr::kBreakdown) {  // the block diagonal is not positive definite, or rho / p . q broke down: no step
    if (h_flags_[kCgFail]) cg_status_last_ = cgnr::kBreakdown;
    SK_HIP_TRY(hipStreamSynchronize(s));
    add_phases(1, 2);
    return SK_OK;
  }

  if (schur()) {  // y_E = V^-1 (b_E - J_E^T (J_F y_F))
    launch_cgnr_jp(cg_jac_, b_y_.p, nullptr, nullptr, b_w_.p, nullptr, s);
    launch_cgnr_eliminate(kCgnrElimBacksub, jac_, cols_e_, b_e_long_slots_.p, b_L_.p, b_b_.p, b_w_.p, b_y_.p, b_e_part_.p, nullptr, s);
  }
  // the model's change from the step itself, the candidate through Plus, its cost
  launch_cgnr_jp(jac_, b_y_.p, nullptr, nullptr, b_w_.p, nullptr, s);
  launch_cgnr_dot(1, b_w_.p, b_r_.p, m_, b_part_.p, nullptr, s);
  launch_cgnr_sum(b_part_.p, (m_ + kCgnrDotChunk - 1) / kCgnrDotChunk, b_scal_.p + kCgModel, nullptr, s);
  launch_cgnr_candidate(dj_.pblocks(), num_pb_, b_y_.p, b_scale_.p, x_, x_new_, b_part_.p, s);
  launch_cgnr_sum(b_part_.p, (num_pb_ + 255) / 256, b_scal_.p + kCgStepSq, nullptr, s);
  SK_HIP_TRY(hipEventRecord(ev_[kEvBacksub], s));
  SK_HIP_TRY(hipMemsetAsync(dj_.fail_flag(), 0, sizeof(int), s));
  int rc = evaluate(x_new_, false);
  if (rc) return rc;
  finish(x_new_, false);
  launch_evaluate_cost(b_cterm_c_.p, nb_, b_part_.p, b_scal_.p + kCgCandCost, s);
  SK_HIP_TRY(hipEventRecord(ev_[kEvCost], s));
  SK_HIP_TRY(hipMemcpyAsync(h_scal_, b_scal_.p, kCgScalCount * sizeof(double), hipMemcpyDeviceToHost, s));
  SK_HIP_TRY(hipMemcpyAsync(h_flags_ + kCgFlagCount, dj_.fail_flag(), sizeof(int), hipMemcpyDeviceToHost, s));
  SK_HIP_TRY(hipStreamSynchronize(s));
  SK_HIP_TRY(hipGetLastError());
  add_phases(1, 4);
  if (!std::isfinite(h_scal_[kCgStepSq]) || !std::isfinite(h_scal_[kCgModel])) return SK_OK;  // invalid step
  out->valid = true;
  out->model_cost_change = -h_scal_[kCgModel];
  out->cost = h_flags_[kCgFlagCount] ? std::numeric_limits<double>::infinity() : h_scal_[kCgCandCost];
  out->step_norm = std::sqrt(h_scal_[kCgStepSq]);
  return SK_OK;
}

int CgnrSolver::write_back() {
  std::vector<double> x((size_t)ng_);
  SK_HIP_TRY(hipMemcpyAsync(x.data(), x_, (size_t)ng_ * sizeof(double), hipMemcpyDeviceToHost, stream_));
  SK_HIP_TRY(hipStreamSynchronize(stream_));
  for (size_t b = 0; b < problem_->block_size.size(); ++b) std::memcpy(problem_->block_ptr[b], &x[plan_.cols.block_off[b]], problem_->block_size[b] * sizeof(double));
  return SK_OK;
}

}  // namespace

std::unique_ptr<SolverBase> make_cgnr_solver(const Options& o, Problem* p) { return std::unique_ptr<SolverBase>(new CgnrSolver(o, p)); }

}  // namespace sk
