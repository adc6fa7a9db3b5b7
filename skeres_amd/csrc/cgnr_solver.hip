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
#include <algorithm>
#include <cmath>
#include <limits>
#include <map>

#include "cgnr_kernels.hpp"
#include "cgnr_plan.hpp"
#include "evaluate_kernels.hpp"
#include "solver.hpp"

namespace sk {
namespace {

static_assert(kCgnrPartSlots == cgnr::kPartSlots, "cgnr_plan.hpp restates common.hpp's constant for the host-only plan");
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
  int write_back() override;
  void describe(Summary* s) override {
    s->num_parameter_blocks = (int)problem_->block_size.size();
    s->num_parameters = plan_.num_ambient; s->num_residual_blocks = (int)problem_->rb_functor.size(); s->num_residuals = plan_.eval.num_rows;
    s->preconditioner_type = opt_.preconditioner_type; s->linear_solver_iterations = n_cg_iterations_;
  }
  bool stat(const std::string& name, double* value) const override {
    if (name == "cg_iterations") { *value = (double)n_cg_iterations_; return true; }
    if (name == "cg_iterations_last") { *value = (double)cg_iterations_last_solve_; return true; }
    if (name == "cg_status_last") { *value = (double)cg_status_last_; return true; }
    if (name == "cg_batches") { *value = (double)n_batches_; return true; }
    if (name == "jacobian_nonzeros") { *value = (double)plan_.eval.num_nonzeros; return true; }
    if (name == "graph_replay") { *value = 0.0; return true; }
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

  CgnrPlan plan_;
  int n_ = 0, ng_ = 0, m_ = 0, nb_ = 0, num_pb_ = 0, update_parts_ = 0;
  std::vector<size_t> member_off_;
  std::map<int, TapeDevBuffers> tapes_dev_;
  // the problem and both plans on the device (uploaded once)
  DevBuf<double> b_consts_, b_stage_;
  DevBuf<size_t> b_const_off_, b_pidx_off_, b_blk_stage_, b_blk_stage_cost_;
  DevBuf<int> b_xoff_, b_blocks_, b_members_, b_blk_stride_, b_blk_dim_, b_blk_loss_, b_row_off_, b_val_off_, b_slot_begin_, b_slot_block_, b_slot_k0_,
      b_slot_pos_, b_slot_owner_, b_slot_col_, b_slot_size_, b_row_block_, b_cb_col_, b_cb_size_, b_cb_moff_, b_cb_slots_, b_part_cb_, b_part_begin_,
      b_part_end_, b_part_out_, b_long_cb_, b_long_begin_, b_flags_, b_fail_;
  DevBuf<ParamBlock> b_pblocks_;
  DevBuf<LossNode> b_nodes_;
  // the state: x and the candidate; the Jacobian's values, residuals and cost terms; the vectors of the tangent space
  DevBuf<double> b_xa_, b_xb_, b_val_, b_r_, b_rc_, b_cterm_, b_cterm_c_, b_scale_, b_gs_, b_b_, b_D2_, b_bsum_, b_L_, b_y_, b_res_, b_z_, b_p_, b_q_, b_w_,
      b_part_, b_jtw_part_, b_bd_part_, b_scal_;
  CgnrJac jac_{};
  CgnrCols cols_{};
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
  int rc = cgnr_plan_build(p, &plan_, &why);
  if (rc != SK_OK) { set_error("%s", why.c_str()); return rc; }
  const EvaluatePlan& E = plan_.eval;
  n_ = plan_.num_cols; ng_ = plan_.num_ambient; m_ = E.num_rows; nb_ = (int)E.blocks.size(); num_pb_ = (int)p.block_ptr.size();
  if (n_ == 0) { set_error("every parameter block is constant: nothing to optimise"); return SK_ERR_INVALID_ARGUMENT; }
  hipStream_t s = stream_;
  auto padded = [](std::vector<int> v) { if (v.empty()) v.push_back(0); return v; };

  // the evaluation's side, as sk_problem_evaluate uploads it
  std::vector<double> x((size_t)ng_);
  for (int b = 0; b < num_pb_; ++b) std::memcpy(&x[plan_.block_off[b]], p.block_ptr[b], p.block_size[b] * sizeof(double));
  std::vector<int> xoff(p.rb_pidx.size());
  for (size_t i = 0; i < p.rb_pidx.size(); ++i) xoff[i] = plan_.block_off[p.rb_pidx[i]];
  std::vector<ParamBlock> pblocks((size_t)num_pb_);
  for (int b = 0; b < num_pb_; ++b) {
    ParamBlock& pb = pblocks[b];
    pb.type = plan_.pb_type[b]; pb.global_size = p.block_size[b]; pb.local_size = plan_.pb_local_size[b]; pb.constant_mask = plan_.pb_mask[b];
    pb.global_off = plan_.block_off[b]; pb.local_off = plan_.pb_local_off[b];
  }
  std::vector<int> blk_dim(nb_, 0), blk_loss(nb_, -1), members;
  for (const EvaluateGroup& G : E.groups) {
    member_off_.push_back(members.size());
    members.insert(members.end(), G.members.begin(), G.members.end());
    for (int i : G.members) blk_dim[i] = G.dim;
    if (G.functor >= kTapeFunctorBase) {  // a recorded functor: its tape goes to the device once
      const Tape& t = *p.tapes[G.functor - kTapeFunctorBase];
      if (tape_pick_width(t, 128) == 0 || tape_lds_bytes(t, 0, 128) > kTapeLdsBudget) {
        set_error("a recorded functor needs %d registers: more than the device interpreter holds", t.num_registers);
        return SK_ERR_UNSUPPORTED;
      }
      SK_HIP_TRY(tapes_dev_[G.functor].upload(t, s));
    }
  }
  for (int i = 0; i < nb_; ++i) blk_loss[i] = p.rb_loss[E.blocks[i]];
  std::vector<double> consts = p.consts; if (consts.empty()) consts.push_back(0.0);
  std::vector<LossNode> nodes = p.loss_nodes;
  if (nodes.empty()) { LossNode t; t.type = kLossTrivial; t.f = t.g = -1; t.depth = 0; t.a = t.b = 0.0; nodes.push_back(t); }
  SK_HIP_TRY(b_xa_.upload(x, s)); SK_HIP_TRY(b_xb_.alloc((size_t)ng_));
  x_ = b_xa_.p; x_new_ = b_xb_.p;
  SK_HIP_TRY(b_consts_.upload(consts, s));
  { std::vector<size_t> co = p.rb_const_off; if (co.empty()) co.push_back(0); SK_HIP_TRY(b_const_off_.upload(co, s)); }
  SK_HIP_TRY(b_pidx_off_.upload(p.rb_pidx_off, s)); SK_HIP_TRY(b_xoff_.upload(padded(xoff), s));
  SK_HIP_TRY(b_blocks_.upload(E.blocks, s)); SK_HIP_TRY(b_members_.upload(padded(members), s));
  SK_HIP_TRY(b_blk_stage_.upload(E.blk_stage, s)); SK_HIP_TRY(b_blk_stage_cost_.upload(plan_.blk_stage_cost, s));
  SK_HIP_TRY(b_blk_stride_.upload(E.blk_stride, s)); SK_HIP_TRY(b_blk_dim_.upload(blk_dim, s)); SK_HIP_TRY(b_blk_loss_.upload(blk_loss, s));
  SK_HIP_TRY(b_row_off_.upload(E.row_off, s)); SK_HIP_TRY(b_val_off_.upload(E.val_off, s)); SK_HIP_TRY(b_slot_begin_.upload(E.slot_begin, s));
  SK_HIP_TRY(b_slot_block_.upload(padded(E.slot_block), s)); SK_HIP_TRY(b_slot_k0_.upload(padded(E.slot_k0), s)); SK_HIP_TRY(b_slot_pos_.upload(padded(E.slot_pos), s));
  SK_HIP_TRY(b_slot_owner_.upload(padded(E.slot_owner), s));
  SK_HIP_TRY(b_pblocks_.upload(pblocks, s)); SK_HIP_TRY(b_nodes_.upload(nodes, s));
  SK_HIP_TRY(b_stage_.alloc(std::max<size_t>(E.stage_size, 1)));
  SK_HIP_TRY(b_val_.alloc((size_t)std::max<long long>(E.num_nonzeros, 1)));
  SK_HIP_TRY(b_r_.alloc((size_t)m_)); SK_HIP_TRY(b_rc_.alloc((size_t)m_)); SK_HIP_TRY(b_cterm_.alloc((size_t)nb_)); SK_HIP_TRY(b_cterm_c_.alloc((size_t)nb_));

  // the solver's side
  SK_HIP_TRY(b_slot_col_.upload(padded(plan_.slot_col), s)); SK_HIP_TRY(b_slot_size_.upload(padded(plan_.slot_size), s));
  SK_HIP_TRY(b_row_block_.upload(plan_.row_block, s));
  SK_HIP_TRY(b_cb_col_.upload(plan_.cb_col, s)); SK_HIP_TRY(b_cb_size_.upload(plan_.cb_size, s)); SK_HIP_TRY(b_cb_moff_.upload(plan_.cb_moff, s));
  SK_HIP_TRY(b_cb_slots_.upload(padded(plan_.cb_slots), s));
  SK_HIP_TRY(b_part_cb_.upload(plan_.part_cb, s)); SK_HIP_TRY(b_part_begin_.upload(plan_.part_begin, s)); SK_HIP_TRY(b_part_end_.upload(plan_.part_end, s));
  SK_HIP_TRY(b_part_out_.upload(plan_.part_out, s));
  SK_HIP_TRY(b_long_cb_.upload(padded(plan_.long_cb), s)); SK_HIP_TRY(b_long_begin_.upload(plan_.long_begin, s));
  const size_t msize = (size_t)plan_.cb_moff.back();
  for (DevBuf<double>* v : {&b_scale_, &b_gs_, &b_b_, &b_D2_, &b_y_, &b_res_, &b_z_, &b_p_, &b_q_}) SK_HIP_TRY(v->alloc((size_t)n_));
  SK_HIP_TRY(b_bsum_.alloc(msize)); SK_HIP_TRY(b_L_.alloc(msize)); SK_HIP_TRY(b_w_.alloc((size_t)m_));
  { std::vector<double> ones((size_t)n_, 1.0); SK_HIP_TRY(hipMemcpyAsync(b_scale_.p, ones.data(), ones.size() * sizeof(double), hipMemcpyHostToDevice, s)); SK_HIP_TRY(hipStreamSynchronize(s)); }
  const int ncb = (int)plan_.cb_col.size();
  update_parts_ = (ncb + kCgnrBlockChunk - 1) / kCgnrBlockChunk;
  const size_t parts = std::max({(size_t)3 * update_parts_, (size_t)(n_ / kCgnrDotChunk + 1), (size_t)(m_ / kCgnrDotChunk + 1), (size_t)(num_pb_ / 256 + 1),
                                 (size_t)(nb_ / kEvaluateSumChunk + 1)});
  SK_HIP_TRY(b_part_.alloc(parts));
  SK_HIP_TRY(b_jtw_part_.alloc(std::max<size_t>((size_t)plan_.num_partials * kCgnrLanes, 1)));
  SK_HIP_TRY(b_bd_part_.alloc(std::max<size_t>((size_t)plan_.num_partials * 256, 1)));
  SK_HIP_TRY(b_scal_.alloc(kCgScalCount)); SK_HIP_TRY(b_scal_.zero(s));
  SK_HIP_TRY(b_flags_.alloc(kCgFlagCount)); SK_HIP_TRY(b_flags_.zero(s)); SK_HIP_TRY(b_fail_.alloc(1)); SK_HIP_TRY(b_fail_.zero(s));
  SK_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_scal_), kCgScalCount * sizeof(double), hipHostMallocDefault));
  SK_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_flags_), (kCgFlagCount + 1) * sizeof(int), hipHostMallocDefault));

  jac_.num_rows = m_; jac_.row_block = b_row_block_.p; jac_.row_off = b_row_off_.p; jac_.val_off = b_val_off_.p; jac_.slot_begin = b_slot_begin_.p;
  jac_.slot_pos = b_slot_pos_.p; jac_.slot_col = b_slot_col_.p; jac_.slot_size = b_slot_size_.p; jac_.slot_owner = b_slot_owner_.p; jac_.values = b_val_.p;
  cols_.num_cb = ncb; cols_.num_parts = (int)plan_.part_cb.size(); cols_.num_long = (int)plan_.long_cb.size();
  cols_.cb_col = b_cb_col_.p; cols_.cb_size = b_cb_size_.p; cols_.cb_moff = b_cb_moff_.p; cols_.cb_slots = b_cb_slots_.p;
  cols_.part_cb = b_part_cb_.p; cols_.part_begin = b_part_begin_.p; cols_.part_end = b_part_end_.p; cols_.part_out = b_part_out_.p;
  cols_.long_cb = b_long_cb_.p; cols_.long_begin = b_long_begin_.p;
  SK_HIP_TRY(hipStreamSynchronize(s));
  return SK_OK;
}

// The evaluation launches of one point: a launch per functor / tape into the staging planes.
int CgnrSolver::evaluate(const double* x_dev, bool jac) {
  const EvaluatePlan& E = plan_.eval;
  EvaluateEvalArgs ea;
  ea.blocks = b_blocks_.p; ea.consts = b_consts_.p; ea.const_off = b_const_off_.p; ea.xoff = b_xoff_.p; ea.pidx_off = b_pidx_off_.p; ea.x = x_dev; ea.fail_flag = b_fail_.p;
  for (size_t g = 0; g < E.groups.size(); ++g) {
    const EvaluateGroup& G = E.groups[g];
    ea.count = (int)G.members.size(); ea.members = b_members_.p + member_off_[g];
    ea.stage = b_stage_.p + (jac ? G.stage_off : plan_.group_stage_cost[g]);
    if (G.functor >= kTapeFunctorBase) {
      if (!launch_evaluate_eval_tape(tapes_dev_[G.functor], jac, ea, stream_)) { set_error("a recorded functor does not fit the device interpreter"); return SK_ERR_UNSUPPORTED; }
    } else {
      launch_evaluate_eval(G.functor, jac, ea, stream_);
    }
  }
  return SK_OK;
}

// Loss correction, projection into the tangent space and the scatter into the values array (jac), or residuals and cost terms alone.
void CgnrSolver::finish(const double* x_dev, bool jac) {
  EvaluateFinishArgs fa;
  fa.num_blocks = nb_; fa.blk_stage = jac ? b_blk_stage_.p : b_blk_stage_cost_.p; fa.blk_stride = b_blk_stride_.p; fa.blk_dim = b_blk_dim_.p; fa.blk_loss = b_blk_loss_.p;
  fa.row_off = b_row_off_.p; fa.val_off = b_val_off_.p; fa.slot_begin = b_slot_begin_.p; fa.slot_block = b_slot_block_.p; fa.slot_k0 = b_slot_k0_.p;
  fa.slot_pos = b_slot_pos_.p; fa.pblocks = b_pblocks_.p; fa.nodes = b_nodes_.p; fa.x = x_dev; fa.stage = b_stage_.p;
  fa.residuals = jac ? b_r_.p : b_rc_.p; fa.values = jac ? b_val_.p : nullptr; fa.cterm = jac ? b_cterm_.p : b_cterm_c_.p;
  launch_evaluate_finish(fa, stream_);
}

int CgnrSolver::evaluate_with_jacobian(bool first) {
  hipStream_t s = stream_;
  SK_HIP_TRY(hipEventRecord(ev_[kEvBegin], s));
  SK_HIP_TRY(hipMemsetAsync(b_fail_.p, 0, sizeof(int), s));
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
  SK_HIP_TRY(hipMemcpyAsync(h_flags_ + kCgFlagCount, b_fail_.p, sizeof(int), hipMemcpyDeviceToHost, s));
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
  launch_cgnr_jp(jac_, b_z_.p, b_p_.p, b_scal_.p, b_w_.p, flags, s);                                                      // w = J p, p = z + beta p
  launch_cgnr_jtw(kCgnrJtwCg, jac_, cols_, b_w_.p, b_D2_.p, b_z_.p, b_p_.p, b_scal_.p, b_q_.p, b_jtw_part_.p, flags, s);   // q = J^T w + D2 p; p stored
  launch_cgnr_dot(0, b_p_.p, b_q_.p, n_, b_part_.p, flags, s);
  launch_cgnr_scalar_alpha(b_part_.p, (n_ + kCgnrDotChunk - 1) / kCgnrDotChunk, b_scal_.p, b_flags_.p, s);                // alpha = rho / p . q
  if (it % cgnr::kResidualResetPeriod == 0) {  // res = b - A x
    launch_cgnr_axpy(b_scal_.p, b_p_.p, b_y_.p, n_, flags, s);
    launch_cgnr_jp(jac_, b_y_.p, nullptr, nullptr, b_w_.p, flags, s);
    launch_cgnr_jtw(kCgnrJtwVector, jac_, cols_, b_w_.p, b_D2_.p, b_y_.p, nullptr, nullptr, b_q_.p, b_jtw_part_.p, flags, s);
    launch_cgnr_update(kCgnrReset, cols_, L, b_b_.p, b_p_.p, b_q_.p, b_scal_.p, b_y_.p, b_res_.p, b_z_.p, b_part_.p, flags, s);
  } else {     // x += alpha p, res -= alpha q
    launch_cgnr_update(kCgnrStep, cols_, L, b_b_.p, b_p_.p, b_q_.p, b_scal_.p, b_y_.p, b_res_.p, b_z_.p, b_part_.p, flags, s);
  }
  launch_cgnr_scalar_end(b_part_.p, update_parts_, opt_.eta, opt_.min_linear_solver_iterations, opt_.max_linear_solver_iterations, b_scal_.p, b_flags_.p, s);
  return SK_OK;
}

int CgnrSolver::linear_solve(double radius, LinearSolve* out) {
  hipStream_t s = stream_;
  *out = LinearSolve();
  ++n_linear_solves_;
  const int max_it = opt_.max_linear_solver_iterations;
  const int batch = dev_knobs().cgnr_batch > 0 ? dev_knobs().cgnr_batch : cgnr::kBatch;
  SK_HIP_TRY(hipEventRecord(ev_[kEvBegin], s));
  SK_HIP_TRY(hipMemsetAsync(b_flags_.p, 0, kCgFlagCount * sizeof(int), s));
  launch_cgnr_precond_factor(cols_, b_bsum_.p, opt_.min_lm_diagonal, opt_.max_lm_diagonal, radius, b_D2_.p, jacobi() ? b_L_.p : nullptr, b_flags_.p, s);
  SK_HIP_TRY(hipEventRecord(ev_[kEvAssemble], s));

  // x = 0, res = b, z = M^-1 res, rho; then iterations in batches until the device says done
  SK_HIP_TRY(hipMemsetAsync(b_y_.p, 0, (size_t)n_ * sizeof(double), s));
  SK_HIP_TRY(hipMemsetAsync(b_p_.p, 0, (size_t)n_ * sizeof(double), s));
  launch_cgnr_update(kCgnrInit, cols_, jacobi() ? b_L_.p : nullptr, b_b_.p, b_p_.p, b_q_.p, b_scal_.p, b_y_.p, b_res_.p, b_z_.p, b_part_.p, nullptr, s);
  launch_cgnr_scalar_init(b_part_.p, update_parts_, b_scal_.p, b_flags_.p, s);
  int enqueued = 0;
  for (;;) {
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

  // the model's change from the step itself, the candidate through Plus, its cost
  launch_cgnr_jp(jac_, b_y_.p, nullptr, nullptr, b_w_.p, nullptr, s);
  launch_cgnr_dot(1, b_w_.p, b_r_.p, m_, b_part_.p, nullptr, s);
  launch_cgnr_sum(b_part_.p, (m_ + kCgnrDotChunk - 1) / kCgnrDotChunk, b_scal_.p + kCgModel, nullptr, s);
  launch_cgnr_candidate(b_pblocks_.p, num_pb_, b_y_.p, b_scale_.p, x_, x_new_, b_part_.p, s);
  launch_cgnr_sum(b_part_.p, (num_pb_ + 255) / 256, b_scal_.p + kCgStepSq, nullptr, s);
  SK_HIP_TRY(hipEventRecord(ev_[kEvBacksub], s));
  SK_HIP_TRY(hipMemsetAsync(b_fail_.p, 0, sizeof(int), s));
  int rc = evaluate(x_new_, false);
  if (rc) return rc;
  finish(x_new_, false);
  launch_evaluate_cost(b_cterm_c_.p, nb_, b_part_.p, b_scal_.p + kCgCandCost, s);
  SK_HIP_TRY(hipEventRecord(ev_[kEvCost], s));
  SK_HIP_TRY(hipMemcpyAsync(h_scal_, b_scal_.p, kCgScalCount * sizeof(double), hipMemcpyDeviceToHost, s));
  SK_HIP_TRY(hipMemcpyAsync(h_flags_ + kCgFlagCount, b_fail_.p, sizeof(int), hipMemcpyDeviceToHost, s));
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
  for (size_t b = 0; b < problem_->block_size.size(); ++b) std::memcpy(problem_->block_ptr[b], &x[plan_.block_off[b]], problem_->block_size[b] * sizeof(double));
  return SK_OK;
}

}  // namespace

std::unique_ptr<SolverBase> make_cgnr_solver(const Options& o, Problem* p) { return std::unique_ptr<SolverBase>(new CgnrSolver(o, p)); }

}  // namespace sk
