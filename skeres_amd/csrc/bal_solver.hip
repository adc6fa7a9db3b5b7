// DENSE_SCHUR path for bundle-adjustment-shaped problems
// (EX/SimpleBundleAdjuster.scala:126-155): every residual block is
// SnavelyReprojectionError on (camera[9], point[3]).  Points are the e-blocks
// that the Schur complement eliminates; the 9C x 9C reduced camera system is
// factored by the MFMA Cholesky.  Multi-GPU: points (and their observations)
// are partitioned over ranks, cameras are replicated, and the reduced system
// is summed with one all-reduce per linear solve.
#include <algorithm>
#include <cmath>
#include <limits>

#include "bal_kernels.hpp"
#include "bal_plan.hpp"
#include "solver.hpp"

namespace sk {

namespace {

// A stream that is capturing when an error makes the enqueueing function return early would fail every later call with
// a capture error instead of the real one: end and discard the capture, and stop replaying graphs for this solver.
struct CaptureGuard {
  hipStream_t s; bool active; bool* graph_mode;
  CaptureGuard(hipStream_t st, bool on, bool* gm) : s(st), active(on), graph_mode(gm) {}
  void release() { active = false; }
  ~CaptureGuard() {
    if (!active) return;
    hipGraph_t g = nullptr;
    (void)hipStreamEndCapture(s, &g);
    if (g) (void)hipGraphDestroy(g);
    (void)hipGetLastError();
    *graph_mode = false;
  }
};

class BalSolver : public SolverBase {
 public:
  BalSolver(const Options& o, Problem* p) : SolverBase(o, p) {}
  // over the fronts of the reduced system (one when it is not dissected); the tail front is factored launch by launch
  double syrk_flops_per_solve() const override {
    double f = 0.0;
    for (int k = 0; k < 3; ++k) if (fr_[k].nblk > 0) f += cholesky_syrk_flops((int)fr_[k].dim, group_, fr_[k].env(), chain_ok() && (k != 1 || tail_chain()), nullptr, fr_[k].ncols, fr_[k].tail_rows, fr_[k].tl());
    return f;
  }
  double syrk_c_bytes_per_solve() const override {
    double tiles = 0.0;
    for (int k = 0; k < 3; ++k) {
      double t = 0.0;
      if (fr_[k].nblk > 0) (void)cholesky_syrk_flops((int)fr_[k].dim, group_, fr_[k].env(), chain_ok() && (k != 1 || tail_chain()), &t, fr_[k].ncols, fr_[k].tail_rows, fr_[k].tl());
      tiles += t;
    }
    return tiles * 2.0 * 128.0 * 128.0 * sizeof(double);
  }
  void set_kernel_timing(int on) override {
    SolverBase::set_kernel_timing(on);
    kt_b_.only(on == 2 ? "gemm_syrk" : ""); kt_b_.enable(on != 0);
  }
  KernelTimer::Stat kernel_stat(const std::string& name) override {
    KernelTimer::Stat a = kt_.get_stat(name), b = kt_b_.get_stat(name);
    a.seconds += b.seconds; a.launches += b.launches;
    return a;
  }
  bool stat(const std::string& name, double* value) const override {
    const int nblk = npad_ / 128;
    if (name == "envelope_fill") {  // 128-blocks that are factored or updated, over the lower triangle of the undissected system
      double in = 0.0;
      for (int k = 0; k < 3; ++k) in += fr_[k].envelope().blocks();  // per block column: the run from the diagonal block down, and the tail rows (right-hand side; a border)
      *value = in / (0.5 * nblk * (nblk + 1.0));
      return true;
    }
    if (name == "reduced_system_blocks") { *value = nblk; return true; }  // (block rows of the undissected reduced system: cameras, pseudo-cameras of retained points, the right-hand side)
    if (name == "camera_order") { *value = camera_order_; return true; }
    if (name == "cholesky_flops_full") { const double n = 9.0 * C_; *value = n * n * n / 3.0; return true; }
    if (name == "cholesky_flops_plan") {
      double f = 0.0;
      for (int k = 0; k < 3; ++k) if (fr_[k].nblk > 0) f += cholesky_plan_flops(fr_[k].nblk, fr_[k].env(), fr_[k].ncols, fr_[k].tail_rows, fr_[k].tl());
      *value = f;
      return true;
    }
    if (name == "cholesky_columns_resident") {
      int r = 0;
      for (int k = 0; k < 3; ++k) {
        if (fr_[k].nblk == 0) continue;
        const CholeskyPlan plan = cholesky_plan(fr_[k].nblk, group_, fr_[k].env(), chain_live() && (k != 1 || tail_chain()), fr_[k].ncols, fr_[k].tail_rows, fr_[k].tl());
        for (char c : plan.resident) r += c ? 1 : 0;
      }
      *value = r;
      return true;
    }
    if (name == "chain_steps") {  // serial steps of the factorisation: block columns, the two leaf fronts of a lock-step dissection counted as one sequence
      *value = (dissected_ ? std::max(fr_[0].ncols, fr_[1].ncols) : 0) + fr_[2].ncols;
      return true;
    }
    if (name == "allreduce_bytes") { *value = (double)packed_elems_ * sizeof(double); return true; }
    if (name == "allreduce_bytes_full_triangle") { *value = (double)tri_packed_elems(nblk) * sizeof(double); return true; }
    if (name == "dissected") { *value = dissected_ ? 1.0 : 0.0; return true; }
    if (name == "pair_segments_short") { *value = d_.num_short_segments; return true; }  // camera pairs of bal_pair_kernel / of bal_pair_long_kernel
    if (name == "pair_segments_long") { *value = d_.num_long_segments; return true; }
    if (name == "graph_replay") { *value = graph_mode_ ? 1.0 : 0.0; return true; }  // the iteration replays as one hipGraph (setup())
    if (name == "host_callback_blocks" || name == "tape_blocks") {  // residual blocks evaluated by the caller's code / by a recorded tape
      const bool host = name == "host_callback_blocks";
      size_t c = 0;
      for (size_t b = 0; b < problem_->rb_functor.size(); ++b)
        c += host ? problem_->rb_functor[b] == SK_FUNCTOR_HOST_CALLBACK : problem_->tape_of_block(b) != nullptr;
      *value = (double)c;
      return true;
    }
    if (name == "tape_width") { *value = tape_mode_ ? bal_tape_width(tape_dev_.host) : 0; return true; }  // derivative slots per pass of the interpreter
    if (name == "tape_lds_bytes") { *value = tape_mode_ ? (double)tape_lds_bytes(tape_dev_.host, bal_tape_width(tape_dev_.host), 256) : 0.0; return true; }
    if (name == "retained_points") { *value = (double)retained_pts_.size(); return true; }
    if (name == "retained_model_us") { *value = retained_model_us_; return true; }
    if (name == "retained_model_us_without") { *value = retained_without_us_; return true; }
    if (name == "border_cameras") { *value = border_cams_; return true; }
    if (name == "border_gap") { *value = border_gap_; return true; }
    if (name == "border_model_us") { *value = border_model_us_; return true; }
    if (name == "border_model_us_plain") { *value = border_plain_us_; return true; }
    if (name == "segments") { *value = segmented_ ? segments_ : (dissected_ ? 2 : 1); return true; }
    if (name == "segment_cameras") { *value = segmented_ ? my_hi_ - my_lo_ : C_; return true; }
    if (name.rfind("model_us_segments_", 0) == 0) { const int k = atoi(name.c_str() + 18); if (k < 1 || k > 8) return false; *value = cut_model_.model_us[k]; return true; }
    if (name == "dissection_head_cameras") { *value = cam_a_; return true; }
    if (name == "dissection_tail_cameras") { *value = cam_b_ - cam_a_; return true; }
    if (name == "dissection_separator_cameras") { *value = dissected_ ? C_ - cam_b_ : 0; return true; }
    if (name == "dissection_model_us_plain") { *value = cut_model_.t_plain; return true; }
    if (name == "dissection_model_us") { *value = cut_model_.t_model; return true; }
    if (name == "model_us_two_segments_with_members") { *value = cut_model_.two_segments_members_us; return true; }
    return strategy_stat(name, value);
  }
  // the grouping is the library's choice (Options::cholesky_group == 0) and the masked streams of the resident panel chain exist
  // ... (the PLAN is then the one with resident runs; whether they really run resident or, with the same grouping, launch
  // by launch — SK_CHOL_CHAIN_SERVER=0, a time-out — is cholesky_factor's business: chain_live())
  bool chain_ok() const { return opt_.cholesky_group == 0 && opt_.lookahead && chol_ctx_.server != nullptr; }
  bool chain_live() const { return chain_ok() && cholesky_chain_enabled(&chol_ctx_); }
  bool tail_chain() const { return chol_ctx_b_.server != nullptr; }  // one device, dissected: the tail front has a resident chain of its own
  int distribution(double* allreduce_s, double* saved_s) const override {
    if (allreduce_s) *allreduce_s = est_allreduce_s_;
    if (saved_s) *saved_s = est_saved_s_;
    return distribution_;
  }

 protected:
  int setup() override;
  int evaluate_with_jacobian(bool first) override;
  // SolverBase's three stepping virtuals.  linear_solve: solve_once, and once more launch by launch after a time-out of the resident
  // panel chain.  The two trials form their candidate and share trial_cost.
  int linear_solve(double radius, LinearSolve* out) override;
  int dogleg_trial(double a, double b, double* cost, double* step_norm) override;
  int bounded_trial(double alpha, double* cost, double* step_norm) override;
  bool supports_dogleg() const override { return true; }
  // One linear solve with what the strategy needs behind its back-substitution: capture or replay, the one synchronisation, the
  // decoding.  What it enqueues is the four stages below, in this order; each records the event that ends its phase.
  int solve_once(double radius, LinearSolve* out, bool* chain_lost);
  struct Backsolve { int resident; bool zero_after; };  // decided once per step, for every front: the resident launch; whether it zeroes what it reads
  int enqueue_schur_assembly(const Backsolve& bs, bool graph);
  int enqueue_factor_backsolve(const Backsolve& bs, bool graph);
  int enqueue_point_backsub(bool graph);
  int enqueue_candidate_cost(int rows, bool* failed);  // rows: 1 the sum of squares, 2 the model term too
  int trial_cost(const double* step_sq_dev, int step_sq_slot, double* cost, double* step_norm);
  const char* refuses_bounds() const override {
    for (int f : problem_->rb_functor)
      if (f == SK_FUNCTOR_HOST_CALLBACK) return "parameter bounds with host-evaluated (director) residual blocks under DENSE_SCHUR are not supported";
    return nullptr;
  }
  int upload_bounds();
  BoundsDev bd_{};
  DevBuf<double> b_bd_box_, b_bd_partial_, b_bd_scal_;
  DoglegDev dl_{};
  DevBuf<double> b_dl_vec_, b_dl_partial_, b_dl_scal_;
  void accept_candidate() override { std::swap(d_.xc, d_.xc_new); std::swap(d_.xp, d_.xp_new); parity_ ^= 1; }
  int write_back() override;
  void describe(Summary* s) override {
    s->num_parameter_blocks = (int)problem_->block_size.size();
    s->num_parameters = problem_->num_parameters();
    s->num_residual_blocks = (int)problem_->rb_functor.size();
    s->num_residuals = problem_->num_residuals;
    s->num_e_blocks = P_total_; s->num_f_blocks = C_ - pseudo_cams_;
  }

 private:
  int gather_rank_scalars(double* vals, int K, const int* ops);
  // director path: the host-evaluated observations at the point held in x_dev ([cameras | points]); jac: with Jacobians
  int host_callbacks(const double* x_dev, bool jac, bool* failed);
  std::vector<int> host_obs_;                 // local observation index of every host-evaluated residual block
  std::vector<const CostFunction*> host_cf_;  // ... and its cost function
  std::vector<double> host_x_, host_rows_h_;
  DevBuf<unsigned char> b_is_host_;
  DevBuf<int> b_host_obs_;
  DevBuf<double> b_host_rows_;
  std::vector<int> h_cam_, h_pt_;             // camera / local point of every local observation (host copy, for the callbacks)
  int gather_rank_scalars_signed(double* vals, int K);
  bool rank_table_on_device(int K) const;
  int enqueue_rank_table(int mode, int K);
  int fold_rank_table(const double* table, double* vals, int K, const int* ops);
  int exchange_rank_table(const double* vals, int K, std::vector<double>* table);

  int C_ = 0, P_total_ = 0, P_ = 0, N_ = 0;   // cameras, all points, local points, local observations
  int res_size_ = 2, cam_size_ = 9, pt_size_ = 3;  // the problem's own (r; c, q) (bal_block_shape): padded to (2; 9, 3) inside
  int n_ = 0, npad_ = 0, rhs_row_ = 0;
  std::vector<int> cam_block_, pt_block_;     // parameter block id of camera i / global point p
  std::vector<int> local_pt_;                 // global point id of local point
  BalDev d_{};
  DevBuf<LossNode> b_loss_nodes_;
  DevBuf<int> b_loss_of_obs_;
  DevBuf<int> b_cam_, b_pt_, b_pt_start_, b_cam_start_, b_cam_obs_, b_obs_slot_, b_seg_start_, b_seg_row_, b_seg_col_, b_pair_row_, b_pair_col_, b_short_segs_, b_long_segs_;
  int *fail_p_ = nullptr, *info_p_ = nullptr;  // device flags: kFail and kInfo of b_scal_ (one reset, one copy back with the scalars)
  DevBuf<double> b_obs_, b_xc_, b_xp_, b_xc_new_, b_xp_new_, b_scale_, b_colsq_, b_gs_, b_step_, b_y_,
      b_r_, b_F_, b_Fcam_, b_E_, b_W_, b_rt_, b_M_, b_q_, b_S_, b_Linv_, b_partial_, b_scal_, b_small_;
  std::vector<int> env_last_;  // block envelope of S (cholesky_factor); empty = dense
  std::vector<int> env_tail_;  // ... and its tail profile when loop-closure cameras are ordered into a trailing border (choose_border); empty = none
  // Retained points (choose_retained_points): not eliminated, three to a pseudo-camera of the reduced system's layout.  C_ includes
  // the pseudo-cameras (cam_block_[i] == -1; no observations, no parameters: inert coordinates); retained_cam_[k] / k % 3: the
  // pseudo-camera (final numbering) and the slot in it of retained point k.
  std::vector<int> retained_pts_, retained_cam_;
  int pseudo_cams_ = 0;
  int border_members_ = 0;  // cameras and pseudo-cameras ordered behind the band (the bordered envelope's border; one device, dissected: the end of the separator)
  double retained_model_us_ = 0.0, retained_without_us_ = 0.0;
  std::vector<int> struct_ocam_, struct_opt_;   // the structure of the reduced system WITH pseudo-cameras (retained_graphs), final numbering; empty: ocam / opt as they are
  int struct_P_ = 0;
  DevBuf<int> b_kept_pt_, b_kept_cam_, b_kept_obs_, b_kept_obs_slot_;
  int P_own_ = 0;  // local points this rank accounts for in |x|^2, max |g| and the write-back: all of them, but for the copies of retained points whose home is another rank (a segmented world; they come last)
  DevBuf<int> b_kept_home_, b_kept_global_;  // per local retained point: 1 = this rank is its home; its index among ALL retained points (the slot of its sums in the small all-reduce)
  DevBuf<int> b_dup_a_, b_dup_b_, b_dup_cam_;  // two residual blocks on one (camera, point) pair: BalDev::dup_*
  int num_dup_ = 0;
  int num_kept_obs_ = 0;
  DevBuf<unsigned char> b_pseudo_;
  int border_cams_ = 0, border_gap_ = 0;          // cameras in that border; the jump in a point's camera list that made a visit
  double border_model_us_ = 0.0, border_plain_us_ = 0.0;
  // The reduced camera system as fronts (FrontHost, bal_plan.hpp): 0 head, 1 tail, 2 root.  Each front is a dense dim x dim matrix inside b_S_.
  FrontHost fr_[3];
  bool dissected_ = false;
  // Several ranks (SK_DISTRIBUTION_SEGMENTED): the camera sequence is cut into segments_ segments with a separator between
  // neighbours; this rank holds ONE leaf front (fr_[0]: segment role_, cameras [my_lo_, my_hi_) of the final numbering)
  // and the root (every separator).  Ranks beyond segments_ replicate rank (r mod segments_) and add zeros to every sum.
  bool segmented_ = false;
  int segments_ = 0, role_ = 0, my_lo_ = 0, my_hi_ = 0;
  bool replica_ = false;
  int fold_world_ = 0;      // ranks whose contributions count in gather_rank_scalars (0: all; segmented: the first segments_)
  int cam_a_ = 0, cam_b_ = 0, border_blocks_ = 0;
  std::vector<int> seg_off_;   // dissected: first camera of every segment in the final numbering, then cam_b_
  std::vector<int> sep_first_; // ... and of every separator, then C_
  std::vector<int> root_last_, root_tail_; // segmented: block envelope of the root (empty: dense — one separator); its tail profile (members of a border behind several separators)
  FrontView leaf_;             // segmented: this rank's leaf front
  DevBuf<int> b_border_row_[2], b_leaf_map_, b_leaf_gmap_;  // separator camera -> row of a leaf's border; border index -> root index (gmap: rhs row -> -1)
  CutModel cut_model_;         // the chain model's figures behind the cut (plan_cuts)
  DissectedSystem ds_;
  CholeskyContext chol_ctx_b_;
  KernelTimer kt_b_;  // launches enqueued by the tail front's own thread
  // Small problems (BASELINE.json configs[1], BAL-49: a reduced system of four 128-blocks) are bound by launch latency:
  // ~60 launches of a few microseconds each per iteration.  Their two launch sequences — the linear solve with the
  // candidate evaluation, and the Jacobian evaluation — are identical from iteration to iteration except for the trust
  // region radius (read from device memory here) and for which of the two parameter buffers is current (`parity_`), so
  // each is captured into a hipGraph once per parity and replayed.
  bool tape_mode_ = false;      // the device functor is a recorded one (tape.hpp), interpreted by the evaluation kernels
  TapeDevBuffers tape_dev_;
  bool graph_mode_ = false;
  int parity_ = 0;
  hipGraphExec_t g_step_[2] = {nullptr, nullptr}, g_eval_[2] = {nullptr, nullptr};
  bool graph_ok() const { return graph_mode_ && !kt_.enabled(); }
  int finish_capture(hipStream_t s, hipGraphExec_t* exec);
  DevBuf<int> b_zero_col0_f_[3], b_mapB_;
  bool mapB_involution_ = false;
  DevBuf<double> b_yf_, b_wf_, b_ybB_;
  double order_hash_ = 0.0;    // of the camera order and the envelope: equal on every rank, or setup() fails
  int camera_order_ = 0;       // which candidate order of the cameras was kept (0 first appearance, 1 memory, 2 RCM)
  int group_ = 3;              // SYRK depth actually used (Options::cholesky_group, or chosen from the envelope)
  DevBuf<double> b_pack_;
  size_t packed_elems_ = 0;
  std::vector<int> pack_col0_h_;            // all-reduce packing: first block column of every block row that travels
  std::vector<long long> pack_off_h_;       // ... and where the row starts in the packed buffer
  DevBuf<int> b_pack_col0_;
  DevBuf<long long> b_pack_off_;
  int distribution_ = SK_DISTRIBUTION_SHARDED;
  double est_allreduce_s_ = 0.0, est_saved_s_ = 0.0;
  int choose_distribution(const std::vector<int>& opt);
  // setup(), stage by stage.  Structure: the residual blocks' cameras and points, in the cameras' numbering of the stage at hand.
  struct Structure {
    std::vector<int> ocam, opt;
    std::vector<int> band_ocam, band_opt;  // retained points: the eliminated points' observations over the real cameras, final numbering (the band a dissection cuts)
    std::vector<int> env_for_model;        // the envelope of the chosen order (whether or not it is then used)
    int Creal = 0;                         // cameras of the problem (C_ grows by the pseudo-cameras of retained points)
  };
  int init_queues();
  int plan_layout(Structure* st);
  void plan_pack();
  int prepare_pack();
  int shard_or_replicate(const std::vector<int>& opt);
  int cut_camera_sequence(Structure* st);
  void adopt_cuts(const CutPlan& cuts, int Cband, bool multi, Structure* st);
  int upload_structure(const LocalStructure& ls);
  int allocate_fronts(const FrontLayout& lay);
  int bind_device_view(const LocalStructure& ls);
  int agree_with_ranks();
  bool distribution_decided_ = false;
  // (SK_DEBUG=setup: where the set-up's wall time goes, one line per stage on stderr)
  std::chrono::steady_clock::time_point setup_t0_, stage_last_;
  void stage(const char* what) {
    if (!dev_knobs().debug_setup) return;
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[skeres_amd] set-up: %-40s %8.1f ms (at %.1f ms)\n", what, std::chrono::duration<double, std::milli>(now - stage_last_).count(),
                 std::chrono::duration<double, std::milli>(now - setup_t0_).count());
    stage_last_ = now;
  }
  CholeskyContext chol_ctx_;
  // The scalars that cross PCIe.  b_scal_ (device, kDevSlots doubles) is copied back to the same slots of h_scal_ (pinned) as one block:
  // [kEvalFirst, kEvalLast] by an evaluation, [kStepFirst, kStepLast] by a step.  The device numbers are the ones the kernels know
  // (bal_pack_rank_scalars_kernel reads them; launch_final_reduce and launch_bal_backsub write runs of two).  Behind the block, h_scal_
  // holds regions that may all be live in one iteration, so none overlaps another.
  enum Slot {
    kGradMaxCam = 0, kXSqCam, kGradMaxPt, kXSqPt, kSumSq,  // evaluation: max |g| and |x|^2 over the cameras (one process: over everything), over this rank's points; sum r^2
    kEvalFirst = kGradMaxCam, kEvalLast = kSumSq,
    kCandSumSq = 0, kModel,                  // step: the candidate's sum r^2, the model term
    kStepSqCam = 8, kStepSqPt,               // ... |delta_c|^2, |delta_p|^2
    kRadiusDev = 12,                         // device only: the radius a replayed graph reads (BalDev::lm_radius_dev)
    kFail = 14, kInfo,                       // two int flags, one double slot each (host_flag): BalDev::fail_flag, the factorisation's info
    kStepFirst = kCandSumSq, kStepLast = kInfo,
    kDevSlots = kStepLast + 1,
    kRadius = kDevSlots,                     // h_scal_ only from here.  The radius: the captured host-to-device copy reads this address at every replay
    kDogleg,                                 // mirror of DoglegDev::scal (DoglegScal)
    kBounds = kDogleg + kDlScalCount,        // mirror of BoundsDev::scal (BoundsScal)
    kRankTable = kBounds + kBdScalCount,     // the table of the ranks' scalars formed on the device: world * K <= kRankTableSlots doubles
    kRankTableSlots = 24,
    kHostSlots = kRankTable + kRankTableSlots
  };
  static_assert(kEvalLast < kStepSqCam && kModel < kStepSqCam && kStepSqPt < kRadiusDev && kRadiusDev < kFail, "b_scal_'s slots are distinct");
  static_assert(kStepLast < kRadius && kRadius < kDogleg && kDogleg + kDlScalCount <= kBounds && kBounds + kBdScalCount <= kRankTable, "h_scal_'s regions do not overlap");
  double* h_scal_ = nullptr;  // pinned, kHostSlots doubles
  int host_flag(int slot) const { int v = 0; std::memcpy(&v, h_scal_ + slot, sizeof(int)); return v; }
  double* rank_table_dev() const { return b_small_.p + 2 * 9 * (size_t)C_ + 6 * retained_pts_.size() + 64; }  // (b_small_: behind the sums of an evaluation)
  int partial_stride_ = 0;
  // The envelope of S has to be zero again before the next assembly (the factor overwrote it).  Round 4: the back-substitution
  // does it — every block of L below the diagonal is read exactly once there, by the owner workgroup of its column, which
  // writes zeros back (cholesky_backsolve(..., zero_after)); what it does not visit, the diagonal 128-blocks and a leaf front's
  // border x border square, is a small pass at the start of the next assembly (b_zero_min_f_: 16-40 MB instead of the envelope's
  // 378 MB on Ladybug-1723).  Rounds 2-3 zeroed the whole envelope on a stream of its own next to the Jacobian evaluation, which
  // that slowed to a third (bal_eval_jac 40 us alone, 116 us beside the zeroing: profiles/r04_point_phases_*).  The full pass
  // remains for a solver without resident kernels, after a factorisation that failed or timed out, and under SK_SCHEDULE_PLAIN.
  bool zero_by_backsolve_ = false;
  bool need_full_zero_ = false;  // the last back-substitution did not (or not surely) zero what it read
  DevBuf<int> b_zero_min_f_[3];
  bool pair_claimed_ = false;  // cholesky_claim_pair_servers: this solver may run a partner front's server beside its own
 public:
  ~BalSolver() override {
    if (pair_claimed_) cholesky_release_pair_servers(&chol_ctx_);
    for (hipGraphExec_t g : {g_step_[0], g_step_[1], g_eval_[0], g_eval_[1]}) if (g) (void)hipGraphExecDestroy(g);
    if (h_scal_) (void)hipHostFree(h_scal_);
  }
};

// Sharding the points pays when the per-iteration work it removes from a rank (evaluation, Schur
// assembly, back-substitution: linear in observations and pair entries) exceeds the all-reduce of the
// reduced system it adds.  The all-reduce is MEASURED here (second and third call of the hook on the real
// buffer); the work is estimated from constants measured on MI355X (chain_model::shardable_work_s).  All ranks
// take the same decision: the measured times are averaged over ranks through the hook itself.
// In replicated mode every rank solves the whole problem with no collective at all (the results are
// bitwise those of one GPU); the speed-up is then 1, which for a small reduced system beats < 1.
int BalSolver::choose_distribution(const std::vector<int>& opt) {
  const int W = opt_.world;
  distribution_ = SK_DISTRIBUTION_SHARDED;
  if (W <= 1 || opt_.distribution_mode == SK_DISTRIBUTION_SHARDED) return SK_OK;
  if (opt_.distribution_mode != SK_DISTRIBUTION_REPLICATED) {
    const double per_iter = chain_model::shardable_work_s(chain_model::pair_entries(opt, P_total_), (double)opt.size());
    est_saved_s_ = per_iter * (1.0 - 1.0 / W);
    int rc = allreduce(b_pack_.p, packed_elems_);  // first call: connection set-up, not timed
    if (rc) return rc;
    SK_HIP_TRY(hipStreamSynchronize(stream_));
    const auto t0 = std::chrono::steady_clock::now();
    for (int rep = 0; rep < 2; ++rep) { rc = allreduce(b_pack_.p, packed_elems_); if (rc) return rc; }
    SK_HIP_TRY(hipStreamSynchronize(stream_));
    double mine = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / 2.0;
    double vals[1] = {mine};
    const int ops[1] = {0};
    SK_HIP_TRY(b_small_.alloc(2 * 9 * (size_t)C_ + 6 * retained_pts_.size() + 64 + 16 * (size_t)W));
    rc = gather_rank_scalars(vals, 1, ops);
    if (rc) return rc;
    est_allreduce_s_ = vals[0] / W;
    collect_allreduce_time(true);
    phase_[5] = 0.0;  // the probe is set-up, not an iteration phase
    if (est_allreduce_s_ <= est_saved_s_) return SK_OK;  // sharding pays
  }
  distribution_ = SK_DISTRIBUTION_REPLICATED;
  opt_.allreduce = nullptr; opt_.world = 1; opt_.rank = 0;
  b_pack_.release();
  return SK_OK;
}

// Set-up, stage by stage (the stage list SK_DEBUG=setup prints).  The host decisions between the collectives are pure functions of
// bal_plan.cpp; every collective (gather_rank_scalars_signed, the hash exchange, choose_distribution's probe, the final agreement)
// is issued here, in one order on every rank.
int BalSolver::setup() {
  setup_t0_ = stage_last_ = std::chrono::steady_clock::now();
  std::string why;
  if (!problem_is_bal_shaped(*problem_, &why)) { set_error("%s", why.c_str()); return SK_ERR_UNSUPPORTED; }
  const Problem& p = *problem_;
  int rc = SK_OK;
  Structure st;
  (void)bal_block_shape(p, &res_size_, &cam_size_, &pt_size_);
  bal_index_problem(p, &cam_block_, &pt_block_, &st.ocam, &st.opt);
  C_ = (int)cam_block_.size(); P_total_ = (int)pt_block_.size();
  st.Creal = C_;
  n_ = 9 * C_; rhs_row_ = n_; npad_ = ((n_ + 1 + 127) / 128) * 128;
  if ((rc = init_queues())) return rc;
  if ((rc = plan_layout(&st))) return rc;
  stage("camera order applied");
  plan_pack();
  if ((rc = cut_camera_sequence(&st))) return rc;
  if (opt_.allreduce && !distribution_decided_) {
    if ((rc = prepare_pack())) return rc;
    if (!segmented_ && (rc = choose_distribution(st.opt))) return rc;
  }
  const LocalInputs li{&st.ocam, &st.opt, C_, P_total_, opt_.world, opt_.rank, segmented_, segments_, role_, &seg_off_, &retained_pts_, &retained_cam_};
  LocalStructure ls = index_local_structure(p, li);
  if (!ls.error.empty()) { set_error("%s", ls.error.c_str()); return SK_ERR_UNSUPPORTED; }
  local_pt_ = ls.local_pt; P_ = ls.P; P_own_ = ls.P_own; N_ = ls.N;
  host_obs_ = ls.host_obs; host_cf_ = ls.host_cf;
  stage("dissection, local observations, camera lists");
  add_pair_lists(&ls, C_, kLongSegment);
  if (!ls.error.empty()) { set_error("%s", ls.error.c_str()); return SK_ERR_UNSUPPORTED; }
  if ((rc = upload_structure(ls))) return rc;
  stage("pair lists, uploads");
  const bool with_pseudo = !struct_ocam_.empty();
  const FrontInputs fi{with_pseudo ? &struct_ocam_ : &st.ocam, with_pseudo ? &struct_opt_ : &st.opt, with_pseudo ? struct_P_ : P_total_, C_, npad_, rhs_row_,
                       &env_last_, &env_tail_, dissected_, segmented_, segments_, role_, &seg_off_, &sep_first_, cam_b_, border_members_, &root_last_, &root_tail_};
  if ((rc = allocate_fronts(layout_fronts(fi)))) return rc;
  stage("fronts, zero pass, tables");
  if ((rc = bind_device_view(ls))) return rc;
  if (bounded_ && (rc = upload_bounds())) return rc;
  if ((rc = agree_with_ranks())) return rc;
  stage("device view, the ranks' agreement");
  return SK_OK;
}

// The factorisation's contexts and the device's queue trial; the ranks' agreement on look-ahead.
int BalSolver::init_queues() {
  const Problem& p = *problem_;
  SK_HIP_TRY(cholesky_init());
  {
    // Launch-bound problems replay their iteration as a hipGraph on ONE stream (below): decided before the look-ahead
    // context exists, so that a reduced system of a few blocks pays neither the queue trial nor its 134 MB of scratch.
    bool host_or_tape = false;
    for (size_t b = 0; b < p.rb_functor.size() && !host_or_tape; ++b) host_or_tape = p.rb_functor[b] == SK_FUNCTOR_HOST_CALLBACK || p.tape_of_block(b) != nullptr;
    if (dogleg() && host_or_tape) {
      for (size_t b = 0; b < p.rb_functor.size(); ++b)
        if (p.rb_functor[b] == SK_FUNCTOR_HOST_CALLBACK) { set_error("DOGLEG with host-evaluated (director) residual blocks under DENSE_SCHUR is not supported"); return SK_ERR_UNSUPPORTED; }
    }
    // (DOGLEG: the captured sequences are Levenberg-Marquardt's — launch by launch)
    graph_mode_ = npad_ / 128 <= 8 && !opt_.allreduce && !host_or_tape && opt_.dissection != SK_DISSECTION_ON && dev_knobs().dissect_at < 0 && opt_.graph_replay && !dogleg() && !bounded_;
    if (graph_mode_) opt_.lookahead = false;  // one stream: the whole iteration is one in-order launch sequence
  }
  chol_ctx_.resident = chol_ctx_b_.resident = opt_.resident_kernels;
  if (opt_.lookahead && chol_ctx_.init() != hipSuccess) {  // CU-masked streams unavailable: plain in-order factorisation
    (void)hipGetLastError();
    opt_.lookahead = false;
  }
  // The device's queue trial (once per device) BEFORE the plans below are chosen: on a device that cannot run the resident panel chain —
  // shared with another process, its kernels serialised — the trial says so, and the lock-step dissection, which exists for that chain,
  // is then not chosen (until round 4 the trial ran after the layout was fixed: two processes sharing one device took the dissected plan
  // launch by launch, 1.9 s per iteration where the undissected one takes 0.2)
  if (opt_.lookahead) cholesky_prepare(&chol_ctx_, stream_);
  if (opt_.allreduce && opt_.world > 1) {
    // the ranks must factor by ONE plan and take ONE distribution decision: a rank without CU-masked streams (no
    // look-ahead, hence no resident chain and no dissection) takes every rank there
    SK_HIP_TRY(b_small_.alloc(2 * 9 * ((size_t)C_ + (size_t)(std::max(1536, opt_.retained_max) + 12) / 3) + 6 * (size_t)(std::max(1536, opt_.retained_max) + 12) + 64 + 16 * (size_t)opt_.world));  // (room for the pseudo-cameras and the retained points' sums the plan below may add)
    double off[1] = {opt_.lookahead ? 0.0 : 1.0};
    int rc = gather_rank_scalars_signed(off, 1);
    if (rc) return rc;
    if (off[0] > 0.0) opt_.lookahead = false;
  }
  return SK_OK;
}

// ---- camera order + block envelope of the reduced system (all ranks' observations: the all-reduced S has the union structure).
// The order is chosen the same way whether or not the envelope is then used (opt_.envelope), so that the two
// settings differ in nothing but the blocks they skip and give bit-identical results. ----
int BalSolver::plan_layout(Structure* st) {
  const Problem& p = *problem_;
  const int Creal = st->Creal;
  // The memory order of the camera blocks (the BAL file's numbering under the reference's layout) is usually the best
  // candidate by far — and host addresses are a process's own: with separately allocated camera blocks it could differ from
  // rank to rank, and the ranks must build the SAME reduced system.  Round 3: the ranks try it and compare (a hash of the
  // order and the envelope: one tiny exchange); only if they disagree do they all fall back to the rank-invariant candidates.
  // (Until then a world of ranks never used it: on the Ladybug-shaped problem the chain model of the best remaining order,
  // reverse Cuthill-McKee, is 12.1 ms against 9.1 — every multi-rank run would have factored a third more slowly.)
  // (the border of loop-closure cameras: not with an explicit dissection or segmentation — the fronts of those have borders of
  // their own kind — and only inside the envelope machinery)
  RetainedGraphs rgraphs;
  // (an explicitly SEGMENTED world takes a border of loop-closure cameras — its members join the one separator — when it is cut in TWO:
  // sk_options_set_max_segments(o, 2); retained points it takes with any number of segments: their pseudo-cameras are a border of the root)
  const bool many_segments = opt_.allreduce && opt_.world > 1 && opt_.distribution_mode == SK_DISTRIBUTION_SEGMENTED && opt_.max_segments != 2;
  const bool border_ok = opt_.envelope && opt_.border != SK_BORDER_OFF && opt_.dissection != SK_DISSECTION_ON && dev_knobs().dissect_at < 0 && !many_segments;
  // (retained points: not with an explicit dissection; a launch-bound problem under hipGraph replay has nothing to gain)
  const bool retained_ok = opt_.retained != SK_RETAINED_OFF && opt_.dissection != SK_DISSECTION_ON && dev_knobs().dissect_at < 0 && !graph_mode_;
  CameraOrderPlan plan;
  auto pick = [&](bool with_memory_order) {
    ReducedSystemPlan rp = plan_reduced_system(p, cam_block_, st->ocam, st->opt, Creal, P_total_, with_memory_order, border_ok, opt_.border,
                                               retained_ok ? opt_.retained : SK_RETAINED_OFF, opt_.retained_max);
    plan = std::move(rp.order);
    retained_pts_ = rp.retained; rgraphs = std::move(rp.graphs);
    retained_without_us_ = rp.without_us; retained_model_us_ = retained_pts_.empty() ? 0.0 : plan.model_us;
    unsigned long long h = 1469598103934665603ull;
    for (int v : retained_pts_) { h ^= (unsigned)v; h *= 1099511628211ull; }
    for (int v : plan.id) { h ^= (unsigned)v; h *= 1099511628211ull; }
    for (int v : plan.last) { h ^= (unsigned)v; h *= 1099511628211ull; }
    for (int v : plan.tail) { h ^= (unsigned)v; h *= 1099511628211ull; }
    order_hash_ = (double)(h >> 12);  // 52 bits: exact in a double
  };
  stage("structure, queue trial");
  pick(true);
  stage("plan of the reduced system");
  if (opt_.allreduce && opt_.world > 1) {
    double v[2] = {order_hash_, -order_hash_};
    int rc = gather_rank_scalars_signed(v, 2);
    if (rc) return rc;
    if (v[0] != order_hash_ || v[1] != -order_hash_) pick(false);  // (every rank sees the disagreement: max and min differ)
  }
  const std::vector<int>& id = plan.id;
  camera_order_ = plan.candidate;
  if (!retained_pts_.empty()) {
    // the reduced system has a pseudo-camera for every three retained points: C_ counts them from here on (cam_block_: -1)
    pseudo_cams_ = rgraphs.Cx - Creal;
    C_ = rgraphs.Cx;
    n_ = 9 * C_; rhs_row_ = n_; npad_ = ((n_ + 1 + 127) / 128) * 128;
    struct_ocam_ = rgraphs.ocam_x; struct_opt_ = rgraphs.opt_x; struct_P_ = rgraphs.Px;
    for (int& c : struct_ocam_) c = id[c];
    st->band_ocam = rgraphs.ocam_g; st->band_opt = rgraphs.opt_g;
    for (int& c : st->band_ocam) c = id[c];
    retained_cam_.resize(retained_pts_.size());
    for (size_t k = 0; k < retained_pts_.size(); ++k) retained_cam_[k] = id[Creal + (int)k / 3];
  }
  std::vector<int> cb(C_, -1);
  for (int c = 0; c < Creal; ++c) cb[id[c]] = cam_block_[c];
  cam_block_.swap(cb);
  for (int& c : st->ocam) c = id[c];
  const int nblk = npad_ / 128;
  const double best = plan.flops, full = cholesky_syrk_flops(npad_, 1, nullptr);
  border_plain_us_ = plan.border.plain_us;
  if (plan.bordered) {
    env_tail_ = plan.tail;
    border_cams_ = plan.border.border_cams; border_gap_ = plan.border.gap;
    border_model_us_ = plan.border.model_us;
  }
  group_ = opt_.group_or(opt_.envelope && best < 0.5 * full ? 1 : 3);
  st->env_for_model = plan.last;
  if (opt_.envelope) env_last_ = plan.last;
  else env_tail_.clear();  // (retained points make a border with or without the envelope: without it every block is factored)
  if (dev_knobs().debug_envelope && opt_.envelope) {
    long h = 0;
    for (int c = 0; c < nblk; ++c) h += env_last_[c] - c;
    std::fprintf(stderr, "[skeres_amd] camera order %d (0 first appearance, 1 memory, 2 RCM); envelope: %d block columns, mean height %.1f; "
                 "trailing-update flops %.3e (full %.3e)\n", camera_order_, nblk, (double)h / nblk, best, full);
    if (border_cams_ > 0)
      std::fprintf(stderr, "[skeres_amd] loop closures: %d cameras in a trailing border (visits split at jumps of more than %d cameras): chain model %.0f us against %.0f\n",
                   border_cams_, border_gap_, border_model_us_, border_plain_us_);
  }
  return SK_OK;
}

// ---- multi-GPU: shard the points, or replicate? ----
// What travels in the all-reduce of the reduced system is the part of its lower block triangle INSIDE the envelope:
// block row kb from the first block column that reaches it (the right-hand-side row whole) — 0.36 GB instead of 0.98 GB
// on the Ladybug-1723-shaped system, exactly the blocks the assembly can write.
static void pack_rows(int nblk, const std::vector<int>& last, const std::vector<int>& tail, std::vector<int>* col0, std::vector<long long>* off) {
  col0->assign(nblk, 0);
  off->assign(nblk + 1, 0);
  if (!last.empty()) *col0 = cholesky_row_first_cols(nblk, last.data(), tail.empty() ? nullptr : tail.data());
  for (int kb = 0; kb < nblk; ++kb) (*off)[kb + 1] = (*off)[kb] + (long long)128 * 128 * (kb + 1 - (*col0)[kb]);
}
void BalSolver::plan_pack() {
  pack_rows(npad_ / 128, env_last_, env_tail_, &pack_col0_h_, &pack_off_h_);
  packed_elems_ = (size_t)pack_off_h_.back();
}
// the buffer the reduced system travels in (the caller's, or our own)
int BalSolver::prepare_pack() {
  if (opt_.reduce_buffer) {
    if (opt_.reduce_buffer_bytes < packed_elems_ * sizeof(double)) { set_error("reduce buffer too small: need %zu bytes", packed_elems_ * sizeof(double)); return SK_ERR_INVALID_ARGUMENT; }
    b_pack_.adopt(static_cast<double*>(opt_.reduce_buffer), packed_elems_);
  } else {
    SK_HIP_TRY(b_pack_.alloc(packed_elems_));
  }
  SK_HIP_TRY(b_pack_.zero(stream_));
  return SK_OK;
}
int BalSolver::shard_or_replicate(const std::vector<int>& opt) {
  int rc = prepare_pack();
  if (rc) return rc;
  rc = choose_distribution(opt);
  if (rc) return rc;
  distribution_decided_ = true;
  return SK_OK;
}

// ---- dissect?  One process: only when forced (measured not to pay on one chip).  Several ranks: the SEGMENTED
// distribution — every rank's device eliminates one segment of the camera sequence — when the model of the chains
// predicts a gain (or when asked for). ----
// Retained points rule out the segmented distribution (their rows couple with every segment), so a world of ranks decides HERE
// between sharding the points and replicating the solve — before the dissection: a rank that replicates is a single device from
// here on (choose_distribution), and takes the lock-step dissection a single device takes
// Round 5: ... unless the world can take the sequence as TWO segments — head and tail on two ranks' devices, the retained points'
// pseudo-cameras (and a border of loop-closure cameras) members of the one separator, exactly the fronts a single device holds side by
// side: tried first (pass 0 below), against what one device would do with the lock-step plan.
int BalSolver::cut_camera_sequence(Structure* st) {
  const bool seg_modes = opt_.distribution_mode == SK_DISTRIBUTION_AUTO || opt_.distribution_mode == SK_DISTRIBUTION_SEGMENTED;
  if (opt_.allreduce && opt_.world > 1 && pseudo_cams_ > 0 && !seg_modes) {
    int rc = shard_or_replicate(st->opt);
    if (rc) return rc;
  }
  for (int pass = 0; pass < 2; ++pass) {
    // (one device: a border — the cameras of loop closures, the pseudo-cameras of retained points — joins the ONE separator, which both
    // fronts border on, and the band in front of it is what is cut; several ranks: a bordered system is not dissected)
    const bool multi = opt_.allreduce != nullptr && opt_.world >= 2;
    border_members_ = env_tail_.empty() ? 0 : border_cams_ + pseudo_cams_;
    const BandStructure band{&st->ocam, &st->opt, C_, P_total_, &st->band_ocam, &st->band_opt, &struct_ocam_, &struct_opt_, struct_P_,
                             &st->env_for_model, &env_tail_, npad_ / 128, pseudo_cams_, border_members_};
    // (a border of loop-closure cameras alone — every point eliminated — is left undissected, as until round 4: the band then keeps its
    // SYRK-bound block columns, which the lock-step cannot pair and the border's rows make dearer; measured on Ladybug-1723 with three
    // places revisited: 8.1-9.2 ms of Cholesky phase for three cuts against 8.2 undissected)
    // ... unless no block column of the bordered band is SYRK-bound to begin with (a sequence of a few hundred cameras)
    const bool band_chain_bound = band_is_chain_bound(band);
    const bool two_seg_try = multi && pseudo_cams_ > 0 && seg_modes && !distribution_decided_;  // (see above)
    const bool pseudo_border = border_members_ > 0 && (!multi || two_seg_try) && (pseudo_cams_ > 0 || band_chain_bound);
    const int Cband = C_ - (pseudo_border ? border_members_ : 0);
    const bool plan_ok = opt_.dissection != SK_DISSECTION_OFF && opt_.envelope && opt_.lookahead && opt_.cholesky_group == 0 && (env_tail_.empty() || pseudo_border);
    bool may_dissect = plan_ok && (multi ? ((pseudo_cams_ == 0 || two_seg_try) && seg_modes)
                                         : (!opt_.allreduce && chol_ctx_b_.init_secondary(chol_ctx_) == hipSuccess));
    if (!may_dissect) (void)hipGetLastError();
    if (!plan_ok && opt_.distribution_mode == SK_DISTRIBUTION_SEGMENTED) {
      set_error("the segmented distribution needs the library's own factorisation plan (envelope, look-ahead, no explicit group); not supported with these options");
      return SK_ERR_UNSUPPORTED;
    }
    CutPlan cuts;
    if (may_dissect) {
      // one device: the lock-step schedule and its own cut
      // (only under the resident chain: the partner front rides in ITS launches — with SK_CHOL_CHAIN_SERVER=0, or on a device that
      // lost its chain, a single device stays undissected)
      const bool lockstep_cut = !multi && opt_.dissection == SK_DISSECTION_AUTO && opt_.resident_kernels && cholesky_chain_enabled(&chol_ctx_);
      const CutFlags flags{multi, two_seg_try, lockstep_cut, pseudo_border, opt_.dissection, opt_.distribution_mode, opt_.max_segments, opt_.world, dev_knobs().dissect_at};
      cuts = plan_cuts(band, flags, &cut_model_);
      if (cuts.needs_pair_claim) {  // (two resident servers per factorisation: the fifth such solver alive on a device stays undissected)
        if (!pair_claimed_) pair_claimed_ = cholesky_claim_pair_servers(&chol_ctx_);
        if (!pair_claimed_ && cuts.drop_without_claim) { cuts.a.clear(); cuts.b.clear(); }
      }
    }
    if (two_seg_try && cuts.a.empty() && opt_.distribution_mode != SK_DISTRIBUTION_SEGMENTED) {
      // no cut that pays: shard the points or replicate (a replicating rank is a single device from here on), then once more
      int rc = shard_or_replicate(st->opt);
      if (rc) return rc;
      continue;
    }
    if (multi && opt_.distribution_mode == SK_DISTRIBUTION_SEGMENTED && cuts.a.empty()) {
      set_error("the segmented distribution needs a separator in the camera sequence (no point seen from both ends); not supported for this problem");
      return SK_ERR_UNSUPPORTED;
    }
    if (!cuts.a.empty()) adopt_cuts(cuts, Cband, multi, st);
    break;
  }
  return SK_OK;
}

void BalSolver::adopt_cuts(const CutPlan& cuts, int Cband, bool multi, Structure* st) {
  dissected_ = true;
  segmented_ = multi;
  const CutNumbering num = apply_cuts(cuts, Cband, C_);
  seg_off_ = num.seg_off; sep_first_ = num.sep_first;
  const std::vector<int>& fin = num.fin;
  segments_ = (int)cuts.a.size() + 1;
  cam_b_ = seg_off_[segments_];
  std::vector<int> cb2(C_);
  for (int c = 0; c < C_; ++c) cb2[fin[c]] = cam_block_[c];
  cam_block_.swap(cb2);
  for (int& c : st->ocam) c = fin[c];
  for (int& c : struct_ocam_) c = fin[c];
  for (int& c : retained_cam_) c = fin[c];
  env_tail_.clear();  // (the fronts have envelopes of their own)
  cam_a_ = seg_off_[1];  // (one device: the head [0, cam_a_), the tail [cam_a_, cam_b_))
  if (!segmented_) return;
  // Rank r < segments_ owns segment r; further ranks are replicas of rank (r mod segments_): they do the same work and
  // add zeros to every sum.  What is exchanged per iteration: the root front (the separators' block-tridiagonal system
  // with the segments' Schur complements), the cameras' column norms and gradient, and a handful of scalars.
  distribution_ = SK_DISTRIBUTION_SEGMENTED;
  role_ = opt_.rank % segments_;
  replica_ = opt_.rank >= segments_;
  fold_world_ = segments_;
  my_lo_ = seg_off_[role_]; my_hi_ = seg_off_[role_ + 1];
  // (the border's members — behind the last separator — are a border of the root too: active from its first block column)
  std::vector<int> sep_off;  // scalar offsets of the separators in the root, then their total
  for (int f : sep_first_) sep_off.push_back(9 * (std::min(f, C_ - border_members_) - cam_b_));
  root_tail_.clear();
  root_last_ = root_envelope(sep_off, 9 * border_members_, &root_tail_);
  pack_rows((9 * (C_ - cam_b_) + 1 + 127) / 128, root_last_, root_tail_, &pack_col0_h_, &pack_off_h_);
  packed_elems_ = (size_t)pack_off_h_.back();
}

// ---- device buffers: this rank's observations, lists and parameter vectors ----
int BalSolver::upload_structure(const LocalStructure& ls) {
  const Problem& p = *problem_;
  hipStream_t s = stream_;
  SK_HIP_TRY(b_cam_.upload(ls.cam, s)); SK_HIP_TRY(b_pt_.upload(ls.pt, s)); SK_HIP_TRY(b_obs_.upload(ls.obs, s));
  if (ls.tape) { tape_mode_ = true; SK_HIP_TRY(tape_dev_.upload(*ls.tape, s)); }
  SK_HIP_TRY(b_pt_start_.upload(ls.pt_start, s)); SK_HIP_TRY(b_cam_start_.upload(ls.cam_start, s)); SK_HIP_TRY(b_cam_obs_.upload(ls.cam_obs, s));
  SK_HIP_TRY(b_obs_slot_.upload(ls.slot, s));
  if (!ls.dup_cam.empty()) { SK_HIP_TRY(b_dup_a_.upload(ls.dup_a, s)); SK_HIP_TRY(b_dup_b_.upload(ls.dup_b, s)); SK_HIP_TRY(b_dup_cam_.upload(ls.dup_cam, s)); }
  num_dup_ = (int)ls.dup_cam.size();
  SK_HIP_TRY(b_seg_start_.upload(ls.seg_start, s)); SK_HIP_TRY(b_seg_row_.upload(ls.seg_row, s)); SK_HIP_TRY(b_seg_col_.upload(ls.seg_col, s));
  SK_HIP_TRY(b_pair_row_.upload(ls.pair_row, s)); SK_HIP_TRY(b_pair_col_.upload(ls.pair_col, s));
  SK_HIP_TRY(b_short_segs_.upload(ls.short_segs, s)); SK_HIP_TRY(b_long_segs_.upload(ls.long_segs, s));
  d_.num_short_segments = (int)ls.short_segs.size(); d_.num_long_segments = (int)ls.long_segs.size();
  const size_t nc = 9 * (size_t)C_, np = 3 * (size_t)P_, nx = nc + np;
  std::vector<double> x(nx, 0.0);  // (the padding coordinates of a smaller shape: zeros, and inert — see free_mask below)
  for (int i = 0; i < C_; ++i) if (cam_block_[i] >= 0) std::memcpy(&x[9 * (size_t)i], p.block_ptr[cam_block_[i]], cam_size_ * sizeof(double));  // (a pseudo-camera: zeros)
  for (int q = 0; q < P_; ++q) std::memcpy(&x[nc + 3 * (size_t)q], p.block_ptr[pt_block_[local_pt_[q]]], pt_size_ * sizeof(double));
  // x vectors are stored [cameras | points] so whole-vector kernels run once
  SK_HIP_TRY(b_xc_.upload(x, s)); SK_HIP_TRY(b_xc_new_.alloc(nx));
  SK_HIP_TRY(b_scale_.alloc(nx)); SK_HIP_TRY(b_colsq_.alloc(nx)); SK_HIP_TRY(b_gs_.alloc(nx)); SK_HIP_TRY(b_step_.alloc(nx));
  {
    // scale starts as the mask of free coordinates: 1, or 0 for a coordinate that is held constant — a constant parameter
    // block (Problem::SetParameterBlockConstant) or the constant coordinates of a SubsetParameterization (ceres.i:186-210);
    // an IdentityParameterization changes nothing.  See jacobi_scale_kernel.
    std::vector<double> free_mask(nx, 1.0);
    auto mask_block = [&](int block, size_t off, int size, int padded) {
      for (int k = size; k < padded; ++k) free_mask[off + k] = 0.0;  // padding of a shape smaller than (2; 9, 3): inert coordinates
      if ((size_t)block < p.block_constant.size() && p.block_constant[block]) { for (int k = 0; k < size; ++k) free_mask[off + k] = 0.0; return; }
      const int pi = (size_t)block < p.block_param.size() ? p.block_param[block] : -1;
      if (pi < 0) return;
      const LocalParameterization& lp = p.params[pi];
      if (lp.type == kParamSubset) for (int k = 0; k < size; ++k) if ((lp.constant_mask >> k) & 1u) free_mask[off + k] = 0.0;
    };
    for (int i = 0; i < C_; ++i) {
      if (cam_block_[i] >= 0) mask_block(cam_block_[i], 9 * (size_t)i, cam_size_, 9);
      else for (int k = 0; k < 9; ++k) free_mask[9 * (size_t)i + k] = 0.0;  // a pseudo-camera's coordinates are nobody's parameters: inert
    }
    for (int q = 0; q < P_; ++q) mask_block(pt_block_[local_pt_[q]], nc + 3 * (size_t)q, pt_size_, 3);
    SK_HIP_TRY(hipMemcpyAsync(b_scale_.p, free_mask.data(), nx * sizeof(double), hipMemcpyHostToDevice, s));
    SK_HIP_TRY(hipStreamSynchronize(s));
  }
  SK_HIP_TRY(b_y_.alloc(npad_ + 128));
  SK_HIP_TRY(b_r_.alloc(2 * (size_t)N_)); SK_HIP_TRY(b_F_.alloc(18 * (size_t)N_)); SK_HIP_TRY(b_Fcam_.alloc(kFcam * (size_t)N_)); SK_HIP_TRY(b_E_.alloc(6 * (size_t)N_));
  SK_HIP_TRY(b_W_.alloc(kWs * (size_t)N_)); SK_HIP_TRY(b_rt_.alloc(5 * (size_t)N_));
  if (res_size_ < 2 || cam_size_ < 9 || pt_size_ < 3) {  // the planes of the padding coordinates / the missing residual row are never written: zero, once
    SK_HIP_TRY(b_r_.zero(s)); SK_HIP_TRY(b_F_.zero(s)); SK_HIP_TRY(b_E_.zero(s));
  }
  SK_HIP_TRY(b_M_.alloc(6 * (size_t)P_)); SK_HIP_TRY(b_q_.alloc(3 * (size_t)P_));
  if (pseudo_cams_ > 0) {
    std::vector<unsigned char> pseudo(C_, 0);
    for (int i = 0; i < C_; ++i) pseudo[i] = cam_block_[i] < 0 ? 1 : 0;
    SK_HIP_TRY(b_pseudo_.upload(pseudo, s));
    SK_HIP_TRY(b_kept_pt_.upload(ls.kept_pt, s)); SK_HIP_TRY(b_kept_cam_.upload(ls.kept_cam, s));
    if (segmented_) { SK_HIP_TRY(b_kept_home_.upload(ls.kept_home, s)); SK_HIP_TRY(b_kept_global_.upload(ls.kept_global, s)); }
    SK_HIP_TRY(b_kept_obs_.upload(ls.kept_obs, s)); SK_HIP_TRY(b_kept_obs_slot_.upload(ls.kept_obs_slot, s));
    num_kept_obs_ = (int)ls.kept_obs.size();
  }
  return SK_OK;
}

// ---- the fronts of the reduced camera system: their matrices, the zero pass's tables, the small buffers ----
int BalSolver::allocate_fronts(const FrontLayout& lay) {
  hipStream_t s = stream_;
  for (int f = 0; f < 3; ++f) fr_[f] = lay.fr[f];
  border_blocks_ = lay.border_blocks;
  {
    const FrontHost& e = fr_[2];  // (the last front: where the buffers end)
    SK_HIP_TRY(b_S_.alloc(e.s_off + e.dim * e.dim));
    SK_HIP_TRY(b_Linv_.alloc(e.linv_off + (size_t)e.ncols * 128 * 128)); SK_HIP_TRY(b_Linv_.zero(s));
    const size_t y_end = e.y_off + e.dim;
    SK_HIP_TRY(b_yf_.alloc(y_end)); SK_HIP_TRY(b_yf_.zero(s)); SK_HIP_TRY(b_wf_.alloc(y_end)); SK_HIP_TRY(b_ybB_.alloc((size_t)std::max(1, border_blocks_) * 128));
  }
  if (opt_.allreduce) { SK_HIP_TRY(b_pack_col0_.upload(pack_col0_h_, s)); SK_HIP_TRY(b_pack_off_.upload(pack_off_h_, s)); }
  cholesky_prepare(&chol_ctx_, s);  // (once per device: which queues the panel, bulk and server streams sit on; nothing without look-ahead)
  if (dissected_ && !segmented_) SK_HIP_TRY(chol_ctx_b_.init_secondary(chol_ctx_));  // (again, now that the queue choice is made: the queues it left over)
  SK_HIP_TRY(b_S_.zero(s));  // once: the blocks outside the envelopes are never touched again
  for (int f = 0; f < 3; ++f) {
    // first block column each block row is zeroed from: the row envelope, widened by the SYRK depth - 1 (inside a
    // group, the lazy updates read every column of the group down to the LAST column's envelope) — and the whole
    // width for the last block row (right-hand side) and without an envelope
    const FrontHost& F = fr_[f];
    if (F.nblk == 0) continue;
    std::vector<int> col0(F.nblk, 0);
    // the widest group of either way to factor (with / without the resident chain, which a timing mode switches off)
    const bool chain_here = chain_ok() && (f != 1 || tail_chain());
    const int widen = F.last.empty() ? 1 : std::max(group_, cholesky_plan_max_group(cholesky_plan(F.nblk, group_, F.last.data(), chain_here, F.ncols, F.tail_rows, F.tl())));
    if (!F.last.empty()) {
      const std::vector<int> first = cholesky_row_first_cols(F.nblk, F.last.data(), F.tl(), F.tail_rows);  // (the tail rows: from column 0, or as the profile has them)
      for (int i = 0; i < F.nblk; ++i) col0[i] = std::max(0, first[i] - (widen - 1));
    }
    SK_HIP_TRY(b_zero_col0_f_[f].upload(col0, s));
    // ... and what the back-substitution leaves to zero: the diagonal block of every factored block column, and from the first border
    // column on in the border's block rows (the Schur complement a leaf front accumulates there)
    std::vector<int> col_min(F.nblk);
    for (int i = 0; i < F.nblk; ++i) col_min[i] = i < F.ncols ? i : F.ncols;
    SK_HIP_TRY(b_zero_min_f_[f].upload(col_min, s));
  }
  for (int f = 0; f < 2; ++f) if (!lay.border_row_h[f].empty()) SK_HIP_TRY(b_border_row_[f].upload(lay.border_row_h[f], s));
  if (segmented_) { SK_HIP_TRY(b_leaf_map_.upload(lay.leaf_map_h, s)); SK_HIP_TRY(b_leaf_gmap_.upload(lay.leaf_gmap_h, s)); }
  if (dissected_ && !segmented_) { SK_HIP_TRY(b_mapB_.upload(lay.mapB, s)); mapB_involution_ = lay.mapB_involution; }
  partial_stride_ = std::max(std::max(std::max(bal_partial_blocks(N_), bal_point_blocks(P_) + 1), (9 * C_ + 255) / 256), 256) + bal_partial_blocks((int)host_obs_.size());  // (+ 1: the retained points' slot)
  SK_HIP_TRY(b_partial_.alloc(4 * (size_t)partial_stride_));
  SK_HIP_TRY(b_scal_.alloc(kDevSlots)); SK_HIP_TRY(b_scal_.zero(s)); SK_HIP_TRY(b_small_.alloc(2 * 9 * (size_t)C_ + 6 * retained_pts_.size() + 64 + 16 * (size_t)opt_.world));
  fail_p_ = reinterpret_cast<int*>(b_scal_.p + kFail); info_p_ = reinterpret_cast<int*>(b_scal_.p + kInfo);
  SK_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_scal_), kHostSlots * sizeof(double), hipHostMallocDefault));
  if (dogleg()) {
    BalDev shape{}; shape.C = C_; shape.P = P_; shape.N = N_;
    const size_t nx = 9 * (size_t)C_ + 3 * (size_t)P_;
    dl_.stride = dogleg_partial_stride(shape);
    SK_HIP_TRY(b_dl_vec_.alloc(2 * nx)); SK_HIP_TRY(b_dl_vec_.zero(s));
    SK_HIP_TRY(b_dl_partial_.alloc(9 * (size_t)dl_.stride)); SK_HIP_TRY(b_dl_partial_.zero(s));
    SK_HIP_TRY(b_dl_scal_.alloc(16)); SK_HIP_TRY(b_dl_scal_.zero(s));
    dl_.s = b_dl_vec_.p; dl_.g = b_dl_vec_.p + nx; dl_.partial = b_dl_partial_.p; dl_.scal = b_dl_scal_.p;
  }
  return SK_OK;
}

// ---- device view ----
int BalSolver::bind_device_view(const LocalStructure& ls) {
  const Problem& p = *problem_;
  hipStream_t s = stream_;
  const size_t nc = 9 * (size_t)C_, nx = nc + 3 * (size_t)P_;
  d_.C = C_; d_.P = P_; d_.N = N_;
  d_.pseudo = pseudo_cams_ > 0 ? b_pseudo_.p : nullptr; d_.num_kept = pseudo_cams_ > 0 ? (int)ls.kept_pt.size() : 0; d_.kept_pt = b_kept_pt_.p; d_.kept_cam = b_kept_cam_.p;
  d_.num_kept_obs = pseudo_cams_ > 0 ? num_kept_obs_ : 0; d_.kept_obs = b_kept_obs_.p; d_.kept_obs_slot = b_kept_obs_slot_.p;
  d_.kept_home = segmented_ && pseudo_cams_ > 0 ? b_kept_home_.p : nullptr; d_.kept_global = segmented_ && pseudo_cams_ > 0 ? b_kept_global_.p : nullptr;
  d_.num_dup = num_dup_; d_.dup_a = b_dup_a_.p; d_.dup_b = b_dup_b_.p; d_.dup_cam = b_dup_cam_.p;
  d_.res_size = res_size_; d_.cam_size = cam_size_; d_.pt_size = pt_size_;
  d_.cam = b_cam_.p; d_.pt = b_pt_.p; d_.obs = b_obs_.p; d_.pt_start = b_pt_start_.p; d_.cam_start = b_cam_start_.p; d_.cam_obs = b_cam_obs_.p; d_.obs_slot = b_obs_slot_.p;
  d_.num_segments = (int)ls.seg_row.size(); d_.seg_start = b_seg_start_.p; d_.seg_row = b_seg_row_.p; d_.seg_col = b_seg_col_.p;
  d_.short_segments = b_short_segs_.p; d_.long_segments = b_long_segs_.p;
  d_.pair_row_obs = b_pair_row_.p; d_.pair_col_obs = b_pair_col_.p;
  d_.xc = b_xc_.p; d_.xp = b_xc_.p + nc; d_.xc_new = b_xc_new_.p; d_.xp_new = b_xc_new_.p + nc;
  d_.scale_c = b_scale_.p; d_.scale_p = b_scale_.p + nc; d_.colsq_c = b_colsq_.p; d_.colsq_p = b_colsq_.p + nc;
  d_.gs_c = b_gs_.p; d_.gs_p = b_gs_.p + nc; d_.step_c = b_step_.p; d_.step_p = b_step_.p + nc;
  d_.y_c = b_y_.p; d_.r = b_r_.p; d_.F = b_F_.p; d_.Fcam = b_Fcam_.p; d_.E = b_E_.p; d_.What = b_W_.p; d_.u = b_rt_.p; d_.M = b_M_.p; d_.q = b_q_.p;
  for (int f = 0; f < 3; ++f) {
    d_.front[f].S = fr_[f].nblk > 0 ? b_S_.p + fr_[f].s_off : nullptr; d_.front[f].ld = (int)fr_[f].dim; d_.front[f].interior = fr_[f].ncols * 128;
    d_.front[f].rhs_row = fr_[f].rhs_row; d_.front[f].border_row = f < 2 ? b_border_row_[f].p : nullptr;
    d_.y_front[f] = b_yf_.p + fr_[f].y_off;
  }
  d_.seg_lo = segmented_ ? my_lo_ : 0; d_.cam_a = segmented_ ? my_hi_ : cam_a_; d_.cam_b = cam_b_;
  d_.S = d_.front[2].S; d_.ld = d_.front[2].ld; d_.rhs_row = fr_[2].rhs_row;
  if (segmented_) {
    const FrontHost& F = fr_[0];
    leaf_.S = d_.front[0].S; leaf_.ld = (long)F.dim; leaf_.nblk = F.nblk; leaf_.ncols = F.ncols; leaf_.last = F.env();
    leaf_.Linv = b_Linv_.p + F.linv_off; leaf_.rhs_row = F.rhs_row; leaf_.tail_rows = F.tail_rows; leaf_.spike = role_ > 0 && role_ + 1 < segments_;
    leaf_.tail = F.tl();  // (two segments with border members in the separator: their rows are a tail profile of the leaf's envelope)
  }
  if (dissected_ && !segmented_) {
    auto view = [&](int f) {
      FrontView v;
      v.S = d_.front[f].S; v.ld = (long)fr_[f].dim; v.nblk = fr_[f].nblk; v.ncols = fr_[f].ncols; v.last = fr_[f].env();
      v.Linv = b_Linv_.p + fr_[f].linv_off; v.rhs_row = fr_[f].rhs_row; v.tail = fr_[f].tl();
      return v;
    };
    ds_.A = view(0); ds_.B = view(1); ds_.R = view(2); ds_.border_blocks = border_blocks_; ds_.mapB = b_mapB_.p; ds_.mapB_involution = mapB_involution_;
  }
  d_.partial = b_partial_.p; d_.partial_stride = partial_stride_; d_.fail_flag = fail_p_;
  d_.loss_nodes = nullptr; d_.loss_root = p.rb_loss.empty() ? -1 : p.rb_loss[0]; d_.loss_of_obs = nullptr;
  {
    // one loss for every residual block (the usual case: SimpleBundleAdjuster shares one trivialLoss, EX/SimpleBundleAdjuster.scala:135),
    // or a loss per block: then every observation carries its own root
    bool mixed = false;
    int any_root = -1;
    for (size_t b = 0; b < p.rb_loss.size(); ++b) { mixed = mixed || p.rb_loss[b] != p.rb_loss[0]; any_root = std::max(any_root, p.rb_loss[b]); }
    if (mixed) {
      std::vector<int> roots(N_);
      for (int o = 0; o < N_; ++o) roots[o] = p.rb_loss[ls.order[o]];
      SK_HIP_TRY(b_loss_of_obs_.upload(roots, s));
      d_.loss_of_obs = b_loss_of_obs_.p; d_.loss_root = any_root;
    }
  }
  if (d_.loss_root >= 0) { SK_HIP_TRY(b_loss_nodes_.upload(p.loss_nodes, s)); d_.loss_nodes = b_loss_nodes_.p; }
  d_.is_host = nullptr; d_.num_host = (int)host_obs_.size(); d_.host_obs = nullptr; d_.host_rows = nullptr;
  if (!host_obs_.empty()) {
    std::vector<unsigned char> flag(N_, 0);
    for (int o : host_obs_) flag[o] = 1;
    SK_HIP_TRY(b_is_host_.upload(flag, s)); SK_HIP_TRY(b_host_obs_.upload(host_obs_, s));
    SK_HIP_TRY(b_host_rows_.alloc(host_obs_.size() * (size_t)kHostRow));
    d_.is_host = b_is_host_.p; d_.host_obs = b_host_obs_.p; d_.host_rows = b_host_rows_.p;
    h_cam_ = ls.cam; h_pt_ = ls.pt;
    host_x_.resize(nx); host_rows_h_.resize(host_obs_.size() * (size_t)kHostRow);
  }
  graph_mode_ = graph_mode_ && host_obs_.empty() && !dissected_ && !tape_mode_;
  zero_by_backsolve_ = !graph_mode_ && !dev_knobs().schedule_plain && opt_.resident_kernels;
  for (int f = 0; f < 3; ++f) if (fr_[f].nblk > 0 && !cholesky_backsolve_resident(fr_[f].nblk)) zero_by_backsolve_ = false;
  SK_HIP_TRY(hipStreamSynchronize(s));
  return SK_OK;
}

// Parameter bounds: the box in the layout of x, and x projected onto it before the first evaluation.
int BalSolver::upload_bounds() {
  const Problem& p = *problem_;
  hipStream_t s = stream_;
  const size_t nc = 9 * (size_t)C_, nx = nc + 3 * (size_t)P_;
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<double> box(2 * nx);
  std::fill(box.begin(), box.begin() + (long)nx, -inf); std::fill(box.begin() + (long)nx, box.end(), inf);
  auto fill = [&](int block, size_t off, int size) {
    for (int k = 0; k < size; ++k) { box[off + k] = p.lower_bound((size_t)block, k); box[nx + off + k] = p.upper_bound((size_t)block, k); }
  };
  for (int i = 0; i < C_; ++i) if (cam_block_[i] >= 0) fill(cam_block_[i], 9 * (size_t)i, cam_size_);
  for (int q = 0; q < P_; ++q) fill(pt_block_[local_pt_[q]], nc + 3 * (size_t)q, pt_size_);
  SK_HIP_TRY(b_bd_box_.upload(box, s));
  bd_.stride = bounds_partial_stride((int)nx);
  SK_HIP_TRY(b_bd_partial_.alloc(6 * (size_t)bd_.stride)); SK_HIP_TRY(b_bd_partial_.zero(s));
  SK_HIP_TRY(b_bd_scal_.alloc(8)); SK_HIP_TRY(b_bd_scal_.zero(s));
  bd_.lo = b_bd_box_.p; bd_.hi = b_bd_box_.p + nx; bd_.partial = b_bd_partial_.p; bd_.scal = b_bd_scal_.p;
  // (a coordinate held constant lies inside its bounds — SolverBase::check_bounds — so the projection leaves it alone)
  launch_box_project(d_.xc, bd_.lo, bd_.hi, (int)nx, s);
  SK_HIP_TRY(hipStreamSynchronize(s));  // (box is pageable)
  return SK_OK;
}

int BalSolver::agree_with_ranks() {
  if (!opt_.allreduce) return SK_OK;
  // every rank derived the camera order and the envelope for itself (from rank-invariant data): they must be the same
  // reduced system, or the all-reduce would sum mismatched matrices
  double v[2] = {order_hash_, -order_hash_};
  int rc = gather_rank_scalars_signed(v, 2);
  if (rc) return rc;
  if (v[0] != order_hash_ || v[1] != -order_hash_) {
    set_error("the ranks derived different camera orders for the reduced system (are the residual blocks added in the same order on every rank?)");
    return SK_ERR_COMM;
  }
  // ... and the same factorisation plan: a rank whose device cannot run the resident panel chain (its queue trial said
  // so: a shared or serialised device) takes every rank to the launch-by-launch plan — replicated factorisations must
  // round alike, or the ranks' parameters drift apart
  double off[1] = {chain_ok() && !chain_live() ? 1.0 : 0.0};
  rc = gather_rank_scalars_signed(off, 1);
  if (rc) return rc;
  if (off[0] > 0.0) cholesky_disable_chain(&chol_ctx_);
  return SK_OK;
}
// The table of the ranks' scalars formed on the DEVICE (bal_pack_rank_scalars_kernel), summed and copied to pinned host memory behind whatever the
// stream holds — the caller synchronises once and folds.  For worlds whose table fits the pinned scalars' spare room.
bool BalSolver::rank_table_on_device(int K) const { return opt_.allreduce != nullptr && opt_.world > 1 && opt_.world * K <= kRankTableSlots; }
int BalSolver::enqueue_rank_table(int mode, int K) {
  double* dev = rank_table_dev();
  launch_bal_pack_rank_scalars(b_scal_.p, dev, opt_.rank, opt_.world, mode, segmented_, stream_);
  int rc = allreduce(dev, (size_t)opt_.world * K);
  if (rc) return rc;
  SK_HIP_TRY(hipMemcpyAsync(h_scal_ + kRankTable, dev, (size_t)opt_.world * K * sizeof(double), hipMemcpyDeviceToHost, stream_));
  return SK_OK;
}
int BalSolver::fold_rank_table(const double* table, double* vals, int K, const int* ops) {
  const int W = opt_.world;
  const int fold = fold_world_ > 0 ? std::min(fold_world_, W) : W;  // (segmented: ranks beyond the first segments_ are replicas)
  for (int k = 0; k < K; ++k) {
    double a = 0.0;
    for (int r = 0; r < fold; ++r) a = ops[k] ? std::max(a, table[(size_t)r * K + k]) : a + table[(size_t)r * K + k];
    vals[k] = a;
  }
  return SK_OK;
}
// The same table from host values: every rank writes its K values into its own row of a world x K table of zeros, the table is
// sum-reduced and brought back (one synchronisation).
int BalSolver::exchange_rank_table(const double* vals, int K, std::vector<double>* table) {
  table->assign((size_t)opt_.world * K, 0.0);
  for (int k = 0; k < K; ++k) (*table)[(size_t)opt_.rank * K + k] = vals[k];
  double* dev = rank_table_dev();
  SK_HIP_TRY(hipMemcpyAsync(dev, table->data(), table->size() * sizeof(double), hipMemcpyHostToDevice, stream_));
  int rc = allreduce(dev, table->size());
  if (rc) return rc;
  SK_HIP_TRY(hipMemcpyAsync(table->data(), dev, table->size() * sizeof(double), hipMemcpyDeviceToHost, stream_));
  SK_HIP_TRY(hipStreamSynchronize(stream_));
  return SK_OK;
}
// max over ranks of each value (values of either sign)
int BalSolver::gather_rank_scalars_signed(double* vals, int K) {
  std::vector<double> table;
  int rc = exchange_rank_table(vals, K, &table);
  if (rc) return rc;
  for (int k = 0; k < K; ++k) {
    double a = table[k];
    for (int r = 1; r < opt_.world; ++r) a = std::max(a, table[(size_t)r * K + k]);
    vals[k] = a;
  }
  return SK_OK;
}
// Combine per-rank scalars: each rank folds the rows in rank order (identical result on every rank; ops: 0 sum, 1 max).
int BalSolver::gather_rank_scalars(double* vals, int K, const int* ops) {
  if (!opt_.allreduce) return SK_OK;
  std::vector<double> table;
  int rc = exchange_rank_table(vals, K, &table);
  return rc ? rc : fold_rank_table(table.data(), vals, K, ops);
}

int BalSolver::evaluate_with_jacobian(bool first) {
  hipStream_t s = stream_;
  const size_t nc = 9 * (size_t)C_, np = 3 * (size_t)P_;
  SK_HIP_TRY(hipEventRecord(ev_[kEvBegin], s));
  const bool graph = graph_ok() && !first;  // (iteration 0 also derives the Jacobi scaling: its own sequence, run once)
  const bool replay = graph && g_eval_[parity_] != nullptr;
  if (graph && !replay && hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) { (void)hipGetLastError(); graph_mode_ = false; return evaluate_with_jacobian(first); }
  CaptureGuard capture(s, graph && !replay, &graph_mode_);  // an early return below must not leave the stream capturing
  if (!replay) {
  kt_.begin("bal_eval_jac", s);
  if (tape_mode_) launch_bal_eval_jac_tape(d_, tape_dev_, s); else launch_bal_eval_jac(d_, s);
  kt_.end("bal_eval_jac", s);
  int nb = bal_partial_blocks(N_);
  if (d_.num_host > 0) {
    bool failed = false;
    int rc = host_callbacks(d_.xc, true, &failed);
    if (rc) return rc;
    if (failed) return SK_ERR_EVALUATION_FAILED;
    nb += launch_bal_host_jac(d_, nb, s);
  }
  kt_.begin("bal_cam_records", s); launch_bal_cam_records(d_, s); kt_.end("bal_cam_records", s);
  kt_.begin("bal_reduce", s); launch_bal_reduce(d_, s); kt_.end("bal_reduce", s);
  if (opt_.allreduce) {  // camera columns are summed over all ranks' observations
    double* buf = b_small_.p;
    // (a segmented world with retained points: their observations are split over the ranks — their column norms and gradient travel too)
    const size_t nk = segmented_ && pseudo_cams_ > 0 ? 6 * retained_pts_.size() : 0;
    if (nk) SK_HIP_TRY(hipMemsetAsync(buf + 2 * nc, 0, nk * sizeof(double), s));
    if (replica_) {  // its sums are rank (r mod segments_)'s over again
      SK_HIP_TRY(hipMemsetAsync(buf, 0, 2 * nc * sizeof(double), s));
    } else {
      SK_HIP_TRY(hipMemcpyAsync(buf, d_.colsq_c, nc * sizeof(double), hipMemcpyDeviceToDevice, s));
      SK_HIP_TRY(hipMemcpyAsync(buf + nc, d_.gs_c, nc * sizeof(double), hipMemcpyDeviceToDevice, s));
      if (nk) launch_bal_kept_sums(d_, buf + 2 * nc, (int)retained_pts_.size(), true, s);
    }
    int rc = allreduce(buf, 2 * nc + nk);
    if (rc) return rc;
    SK_HIP_TRY(hipMemcpyAsync(d_.colsq_c, buf, nc * sizeof(double), hipMemcpyDeviceToDevice, s));
    SK_HIP_TRY(hipMemcpyAsync(d_.gs_c, buf + nc, nc * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (nk) launch_bal_kept_sums(d_, buf + 2 * nc, (int)retained_pts_.size(), false, s);
  }
  if (first && opt_.jacobi_scaling) {
    launch_jacobi_scale(b_colsq_.p, b_scale_.p, (int)(nc + np), s);
    launch_bal_scale_jac(d_, s);
    launch_bal_cam_records(d_, s);  // F changed under the records
    launch_apply_scale_to_reductions(b_colsq_.p, b_gs_.p, b_scale_.p, (int)(nc + np), s);
  }
  // scalars: sum r^2 ; gradient max-norm and |x|^2 (cameras once, points local)
  if (!opt_.allreduce) {
    // one process: cameras and points as ONE vector ([cameras | points] in every buffer), and the three reductions — sum r^2,
    // max |g|, |x|^2 — in one launch (round 4: five launches of ~6 us each became two)
    const int g = launch_grad_max_xnorm(b_gs_.p, b_scale_.p, d_.xc, (int)(nc + np), b_partial_.p + (size_t)partial_stride_, partial_stride_, s);
    // (under bounds the gradient test is the projected gradient's: below, in a launch of its own — this one's maximum is read for its
    // finiteness alone: a Jacobian entry that is not finite fails the evaluation)
    // (kGradMaxPt and kXSqPt, the points' share in a world of ranks, stay zero: it is inside the cameras' slots here)
    ReduceRows rows;
    rows.n = 3;
    rows.row[0] = 0; rows.count[0] = nb; rows.out[0] = b_scal_.p + kSumSq;
    rows.row[1] = 1; rows.count[1] = g; rows.is_max[1] = 1; rows.out[1] = b_scal_.p + kGradMaxCam;
    rows.row[2] = 2; rows.count[2] = g; rows.out[2] = b_scal_.p + kXSqCam;
    launch_final_reduce_rows(b_partial_.p, partial_stride_, rows, s);
  } else {
  launch_final_reduce(b_partial_.p, partial_stride_, nb, 1, 0, b_scal_.p + kSumSq, s);
  // cameras: every rank holds all of them — but in a segmented world only its own segment's (and the separator's) are
  // current, and the separator's |x|^2 must be counted once: the head's rank takes it
  int c_lo = 0, c_n = (int)nc;
  if (segmented_) { c_lo = 9 * my_lo_; c_n = 9 * (my_hi_ - my_lo_); }
  int gc = launch_grad_max_xnorm(d_.gs_c + c_lo, d_.scale_c + c_lo, d_.xc + c_lo, c_n, b_partial_.p, partial_stride_, s);
  if (segmented_ && role_ == 0) {  // + the separators (slots behind the segment's)
    const int lo2 = 9 * cam_b_, n2 = (int)nc - lo2;
    gc += launch_grad_max_xnorm(d_.gs_c + lo2, d_.scale_c + lo2, d_.xc + lo2, n2, b_partial_.p + gc, partial_stride_, s);
  }
  launch_final_reduce(b_partial_.p, partial_stride_, gc, 2, 1, b_scal_.p + kGradMaxCam, s);
  // (the points this rank accounts for: all its own — not the copies of retained points whose home is another rank, which come last)
  const int np_own = 3 * P_own_;
  const int gp = launch_grad_max_xnorm(d_.gs_p, d_.scale_p, d_.xp, np_own, b_partial_.p + 2 * (size_t)partial_stride_, partial_stride_, s);
  launch_final_reduce(b_partial_.p + 2 * (size_t)partial_stride_, partial_stride_, np_own ? gp : 0, 2, 1, b_scal_.p + kGradMaxPt, s);
  }
  SK_HIP_TRY(hipMemcpyAsync(h_scal_ + kEvalFirst, b_scal_.p + kEvalFirst, (kEvalLast + 1 - kEvalFirst) * sizeof(double), hipMemcpyDeviceToHost, s));
  if (bounded_) {  // max |x - P(x - g)|, |x|^2 and the active bounds in one launch (one device: the whole vector)
    kt_.begin("bounded_grad_max_xnorm", s); launch_bounded_grad_max_xnorm(b_gs_.p, b_scale_.p, d_.xc, (int)(nc + np), bd_, s); kt_.end("bounded_grad_max_xnorm", s);
    SK_HIP_TRY(hipMemcpyAsync(h_scal_ + kBounds + kBdGradMax, bd_.scal + kBdGradMax, (kBdActive + 1 - kBdGradMax) * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  }
  if (graph) {
    if (!replay) { capture.release(); int rc = finish_capture(s, &g_eval_[parity_]); if (rc) return rc; if (!graph_mode_) return evaluate_with_jacobian(first); }
    SK_HIP_TRY(hipGraphLaunch(g_eval_[parity_], s));
  }
  SK_HIP_TRY(hipEventRecord(ev_[kEvJac], s));
  // a world of ranks: the table of the ranks' scalars is formed on the device and summed BEFORE the one host synchronisation (round 5;
  // until then: synchronise, pack on the host, copy up, all-reduce, copy down, synchronise again)
  const bool dev_gather = rank_table_on_device(3) && !graph;
  if (dev_gather) { int rc = enqueue_rank_table(0, 3); if (rc) return rc; }
  SK_HIP_TRY(hipStreamSynchronize(s));
  const double sumsq = h_scal_[kSumSq];
  const double gmax_c = h_scal_[kGradMaxCam], x2_c = h_scal_[kXSqCam];
  // local: sum r^2, max |g_p|, |x_p|^2 — and in a segmented world this rank's cameras' share of max |g_c| and |x_c|^2 too
  double loc[3] = {sumsq, segmented_ ? std::max(h_scal_[kGradMaxPt], gmax_c) : h_scal_[kGradMaxPt], h_scal_[kXSqPt] + (segmented_ ? x2_c : 0.0)};
  const int ops3[3] = {0, 1, 0};
  int rc = dev_gather ? fold_rank_table(h_scal_ + kRankTable, loc, 3, ops3) : gather_rank_scalars(loc, 3, ops3);
  if (rc) return rc;
  add_phases(0, 0);
  cost_ = 0.5 * loc[0];
  gmax_ = segmented_ ? loc[1] : std::max(gmax_c, loc[1]);
  xnorm_ = std::sqrt((segmented_ ? 0.0 : x2_c) + loc[2]);
  if (bounded_) { gmax_ = h_scal_[kBounds + kBdGradMax]; active_bounds_ = (long)h_scal_[kBounds + kBdActive]; }
  // (the maximum keeps a NaN on the device: a Jacobian entry that is not finite fails the evaluation like a residual that is not, as in Ceres.
  // One device only: in a world of ranks a segment's maximum is its own, and a rank that failed alone would leave the others in the next
  // collective; there the decision stays with the cost, which every rank has summed.)
  if (!std::isfinite(cost_) || (!opt_.allreduce && (!std::isfinite(gmax_c) || !std::isfinite(loc[1])))) return SK_ERR_EVALUATION_FAILED;
  return SK_OK;
}

// A time-out of the resident panel chain (info == 2: the device is shared, or its kernels are being serialised) loses
// that factorisation, not the step: the chain is switched off for the device and the same linear system is assembled
// and factored again, launch by launch, in the same iteration — the trajectory does not change.
int BalSolver::linear_solve(double radius, LinearSolve* out) {
  bool chain_lost = false;
  int rc = solve_once(radius, out, &chain_lost);
  if (rc == SK_OK && chain_lost) rc = solve_once(radius, out, &chain_lost);
  return rc;
}

int BalSolver::solve_once(double radius, LinearSolve* out, bool* chain_lost) {
  hipStream_t s = stream_;
  *chain_lost = false;
  *out = LinearSolve();
  ++n_linear_solves_;
  SK_HIP_TRY(hipEventRecord(ev_[kEvBegin], s));
  const bool graph = graph_ok();
  const bool replay = graph && g_step_[parity_] != nullptr;
  bool candidate_failed = false;  // a cost function that cannot be evaluated at the candidate: the step is rejected (cost = max)
  if (graph) {
    h_scal_[kRadius] = radius;  // pinned: the captured host-to-device copy reads it when the graph RUNS
    if (!replay && hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) { (void)hipGetLastError(); graph_mode_ = false; return solve_once(radius, out, chain_lost); }
  }
  CaptureGuard capture(s, graph && !replay, &graph_mode_);
  if (!replay) {
    // the LM diagonal is formed where it is used (bal_lm_diag): the radius travels in the kernel arguments, or — a replayed graph —
    // through device memory
    d_.lm_lo = opt_.min_lm_diagonal; d_.lm_hi = opt_.max_lm_diagonal; d_.lm_radius = radius; d_.lm_radius_dev = nullptr;
    if (graph) {
      SK_HIP_TRY(hipMemcpyAsync(b_scal_.p + kRadiusDev, h_scal_ + kRadius, sizeof(double), hipMemcpyHostToDevice, s));
      d_.lm_radius_dev = b_scal_.p + kRadiusDev;
    }
    // (this step's back-substitution zeroes what it reads when it is the resident launch: decided here, once, for the whole step)
    // (... and whether the back-substitutions of this step are the resident launch at all: one decision for every front — the process-wide
    // switch can be cleared by another solver's time-out at any moment)
    Backsolve bs;
    bs.resident = opt_.resident_kernels && cholesky_backsolve_resident(npad_ / 128) ? 1 : 0;
    bs.zero_after = zero_by_backsolve_ && bs.resident;
    int rc = enqueue_schur_assembly(bs, graph);
    if (rc == SK_OK) rc = enqueue_factor_backsolve(bs, graph);
    if (rc == SK_OK) rc = enqueue_point_backsub(graph);
    if (rc == SK_OK && !dogleg()) rc = enqueue_candidate_cost(2, &candidate_failed);  // (DOGLEG: the candidate is formed and evaluated by dogleg_trial)
    if (rc) return rc;
    if (!graph) SK_HIP_TRY(hipEventRecord(ev_[kEvCost], s));
    SK_HIP_TRY(hipMemcpyAsync(h_scal_ + kStepFirst, b_scal_.p + kStepFirst, (kStepLast + 1 - kStepFirst) * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  const bool dev_gather = rank_table_on_device(4) && !graph;  // (see evaluate_with_jacobian)
  if (dev_gather) { int rc = enqueue_rank_table(1, 4); if (rc) return rc; }
  if (graph) {
    if (!replay) { capture.release(); int rc = finish_capture(s, &g_step_[parity_]); if (rc) return rc; if (!graph_mode_) return solve_once(radius, out, chain_lost); }
    SK_HIP_TRY(hipGraphLaunch(g_step_[parity_], s));
    SK_HIP_TRY(hipEventRecord(ev_[kEvCost], s));
  }
  SK_HIP_TRY(hipStreamSynchronize(s));
  if (graph) {  // one replayed graph: no events inside it — the whole linear solve + candidate evaluation is reported as "factor"
    add_phase(2, ev_[kEvBegin], ev_[kEvCost]);
  } else {
    add_phases(1, 4);
  }
  const int fail = host_flag(kFail), info = host_flag(kInfo);
  if (info != 0) need_full_zero_ = true;  // (a pivot that was not positive, a wait that gave up: whatever the back-substitution did, start from a clean envelope)
  if (cholesky_note_info(opt_.lookahead ? &chol_ctx_ : nullptr, info) && !opt_.allreduce) {  // factor again, launch by launch
    if (graph_mode_) {
      // a replayed graph would launch the resident kernel that has just timed out again and again (the choice is made at capture): the
      // iteration is enqueued launch by launch from here on
      for (hipGraphExec_t* g : {&g_step_[0], &g_step_[1], &g_eval_[0], &g_eval_[1]}) if (*g) { (void)hipGraphExecDestroy(*g); *g = nullptr; }
      graph_mode_ = false;
    }
    *chain_lost = true;
    return SK_OK;
  }
  if (dogleg()) {  // (one device.  Not valid: a pivot or a point block's 3 x 3 was not positive — the damped system is not positive definite at this mu)
    out->valid = (fail | info) == 0;
    out->dl = dogleg::Scalars::from(h_scal_ + kDogleg + kDlScalars);
    return SK_OK;
  }
  // sum r_new^2, model term, |delta_p|^2 (segmented: + this rank's cameras' |delta_c|^2, which no other rank has), failure
  double loc[4] = {h_scal_[kCandSumSq], h_scal_[kModel], h_scal_[kStepSqPt] + (segmented_ ? h_scal_[kStepSqCam] : 0.0), (double)(fail | info)};
  const int ops4[4] = {0, 0, 0, 1};
  int rc = dev_gather ? fold_rank_table(h_scal_ + kRankTable, loc, 4, ops4) : gather_rank_scalars(loc, 4, ops4);
  if (rc) return rc;
  if (opt_.allreduce && loc[3] >= 2.0) cholesky_disable_chain(&chol_ctx_);  // a rank's chain timed out (info == 2): launch by launch on every rank from here on
  const double step_sq = (segmented_ ? 0.0 : h_scal_[kStepSqCam]) + loc[2];
  if (loc[3] != 0.0 || !std::isfinite(step_sq) || !std::isfinite(loc[1])) return SK_OK;  // invalid step
  out->valid = true;
  out->model_cost_change = -loc[1];
  out->cost = candidate_failed ? std::numeric_limits<double>::max() : 0.5 * loc[0];
  out->step_norm = std::sqrt(bounded_ ? h_scal_[kBounds + kBdStepSq] : step_sq);
  out->g_delta = h_scal_[kBounds + kBdGDelta]; out->max_delta = h_scal_[kBounds + kBdMaxDelta];  // (of this solve under bounds only, where they are read)
  return SK_OK;
}

// ---- B. Schur complement assembly ----
int BalSolver::enqueue_schur_assembly(const Backsolve& bs, bool graph) {
  hipStream_t s = stream_;
  kt_.begin("memset_S", s);
  for (int f = 0; f < 3; ++f)
    if (fr_[f].nblk > 0) launch_zero_envelope(d_.front[f].S, (int)fr_[f].dim, (zero_by_backsolve_ && !need_full_zero_) ? b_zero_min_f_[f].p : b_zero_col0_f_[f].p, fr_[f].nblk, s);
  kt_.end("memset_S", s);
  need_full_zero_ = !bs.zero_after;
  SK_HIP_TRY(hipMemsetAsync(b_scal_.p + kFail, 0, (kInfo + 1 - kFail) * sizeof(double), s));  // the failure flag and the factorisation's info
  launch_bal_point_block(d_, s);
  launch_bal_kept_points(d_, s);  // (retained points: their rows of the reduced system; nothing of theirs enters the Schur complement)
  launch_bal_obs_precompute(d_, s);
  kt_.begin("bal_cam_diag", s); launch_bal_cam_diag(d_, s); kt_.end("bal_cam_diag", s);
  kt_.begin("bal_pair", s); launch_bal_pair(d_, s); kt_.end("bal_pair", s);
  if (opt_.allreduce && !segmented_) {  // (segmented: the root front is summed after the leaf has been factored)
    // sum S (with the rhs row) over ranks: only its lower block triangle travels (half the bytes)
    launch_tri_pack(d_.S, npad_, b_pack_.p, npad_ / 128, b_pack_col0_.p, b_pack_off_.p, true, s);  // (never dissected here: front[2] is the whole system)
    int rc = allreduce(b_pack_.p, packed_elems_);
    if (rc) return rc;
    launch_tri_pack(d_.S, npad_, b_pack_.p, npad_ / 128, b_pack_col0_.p, b_pack_off_.p, false, s);
  }
  // D_c^2 onto the cameras' diagonal entries; the padded tails of the interiors and of the root are identities, and the
  // augmented right-hand-side row of the root gets a huge diagonal so that its factorisation stays positive definite (the
  // entry itself is unused; in a leaf's border that diagonal stays zero: it is ADDED to the root's)
  if (!segmented_) {
    // one launch: D^2 of every camera, the identities on the leaf fronts' padding, the root's two diagonal ranges
    BalFinishRanges r;
    int k = 0;
    for (int f = 0; f < 2; ++f)
      if (fr_[f].nblk > 0 && fr_[f].ncols * 128 > 9 * fr_[f].cams) { r.S[k] = d_.front[f].S; r.ld[k] = (int)fr_[f].dim; r.from[k] = 9 * fr_[f].cams; r.to[k] = fr_[f].ncols * 128; r.value[k] = 1.0; ++k; }
    r.S[k] = d_.front[2].S; r.ld[k] = (int)fr_[2].dim; r.from[k] = fr_[2].rhs_row; r.to[k] = fr_[2].rhs_row + 1; r.value[k] = 1e300; ++k;
    if ((int)fr_[2].dim > fr_[2].rhs_row + 1) { r.S[k] = d_.front[2].S; r.ld[k] = (int)fr_[2].dim; r.from[k] = fr_[2].rhs_row + 1; r.to[k] = (int)fr_[2].dim; r.value[k] = 1.0; ++k; }
    launch_bal_finish_all(d_, r, s);
  } else {
    launch_bal_finish_S(d_, 3, s);
    for (int f = 0; f < 2; ++f)
      if (fr_[f].nblk > 0) launch_set_diagonal(d_.front[f].S, (int)fr_[f].dim, 9 * fr_[f].cams, fr_[f].ncols * 128, 1.0, s);
    // (the root's D^2 and diagonals: after the ranks' root fronts have been summed — they are added once)
  }
  if (!graph) SK_HIP_TRY(hipEventRecord(ev_[kEvAssemble], s));
  return SK_OK;
}

// ---- C. dense Cholesky + solves: segmented over ranks, dissected on one device, or a single front ----
int BalSolver::enqueue_factor_backsolve(const Backsolve& bs, bool graph) {
  hipStream_t s = stream_;
  CholeskyContext* ctx = opt_.lookahead ? &chol_ctx_ : nullptr;
  int* bs_info = bs.resident ? info_p_ : nullptr;  // (nullptr: the back-substitutions one launch per block step — nothing resident, nothing that waits)
  double* yf[3] = {b_yf_.p + fr_[0].y_off, b_yf_.p + fr_[1].y_off, b_yf_.p + fr_[2].y_off};
  double* wf[3] = {b_wf_.p + fr_[0].y_off, b_wf_.p + fr_[1].y_off, b_wf_.p + fr_[2].y_off};
  // (the resident back-substitutions find their "not there yet" pattern in every front's y already: one fill here, in front of the
  // factorisation, instead of one in front of each of them, between the factorisation's end and the first hop)
  const bool prefilled = bs.resident != 0;
  if (prefilled) SK_HIP_TRY(hipMemsetAsync(b_yf_.p, 0xff, (fr_[0].dim + fr_[1].dim + fr_[2].dim) * sizeof(double), s));
  if (segmented_) {
    // this rank's segment: factor its interior, leave its Schur complement on the separators next to it; sum the root
    // fronts over the ranks (the separators' own blocks come from whichever rank owns the point, the Schur complements
    // from the segments on either side); then every rank factors the same root and solves its own interior
    const FrontView& L = leaf_;
    const FrontHost& R = fr_[2];
    double* Rs = d_.front[2].S;
    double* RLinv = b_Linv_.p + R.linv_off;
    if (L.ncols > 0) {
      cholesky_factor(L.S, L.ld, L.nblk * 128, L.Linv, info_p_, group_, s, ctx, &kt_, L.last, chain_ok(), L.ncols, L.tail_rows, nullptr, L.tail);
      cholesky_border_add(Rs, (long)R.dim, L.S, L.ld, L.ncols, L.nblk - L.ncols, b_leaf_map_.p, s);
    }
    if (replica_) SK_HIP_TRY(hipMemsetAsync(b_pack_.p, 0, packed_elems_ * sizeof(double), s));  // a replica adds nothing
    else launch_tri_pack(Rs, (int)R.dim, b_pack_.p, R.nblk, b_pack_col0_.p, b_pack_off_.p, true, s);
    int rc = allreduce(b_pack_.p, packed_elems_);
    if (rc) return rc;
    launch_tri_pack(Rs, (int)R.dim, b_pack_.p, R.nblk, b_pack_col0_.p, b_pack_off_.p, false, s);
    // the root's D^2, its right-hand-side row's huge diagonal, the identity on its padding: once, on the sum
    launch_bal_finish_S(d_, 4, s);
    launch_set_diagonal(Rs, (int)R.dim, R.rhs_row, R.rhs_row + 1, 1e300, s);
    launch_set_diagonal(Rs, (int)R.dim, R.rhs_row + 1, (int)R.dim, 1.0, s);
    cholesky_factor(Rs, (long)R.dim, (int)R.dim, RLinv, info_p_, group_, s, ctx, &kt_, R.env(), chain_ok(), -1, 1, nullptr, R.tl());
    cholesky_backsolve(Rs, (long)R.dim, 9 * R.cams, (int)R.dim, R.rhs_row, RLinv, wf[2], yf[2], s, &kt_, R.env(), bs_info, R.tl(), bs.zero_after, bs.resident, prefilled);
    if (L.ncols > 0) {
      cholesky_gather_map(yf[2], b_leaf_gmap_.p, b_ybB_.p, (L.nblk - L.ncols) * 128, s);
      cholesky_backsolve_front(L.S, L.ld, L.nblk, L.ncols, L.rhs_row, L.Linv, b_ybB_.p, wf[0], yf[0], s, L.last, L.spike, L.tail_rows, bs_info, bs.zero_after, L.tail, nullptr, bs.resident, prefilled);
    }
  } else if (dissected_) {
    cholesky_dissected_factor(ds_, info_p_, group_, s, ctx, &chol_ctx_b_, &kt_, &kt_b_, chain_ok());
    cholesky_dissected_backsolve(ds_, 9 * fr_[2].cams, wf[2], yf[2], wf[0], yf[0], wf[1], yf[1], b_ybB_.p, s, &chol_ctx_b_, &kt_, bs_info, bs.zero_after, bs.resident, prefilled);
  } else {
    const FrontHost& R = fr_[2];
    cholesky_factor(d_.front[2].S, (long)R.dim, (int)R.dim, b_Linv_.p, info_p_, group_, s, ctx, &kt_, R.env(), chain_ok(), -1, 1, nullptr, R.tl());
    cholesky_backsolve(d_.front[2].S, (long)R.dim, n_, (int)R.dim, R.rhs_row, b_Linv_.p, wf[2], yf[2], s, &kt_, R.env(), bs_info, R.tl(), bs.zero_after, bs.resident, prefilled);
  }
  if (!graph) SK_HIP_TRY(hipEventRecord(ev_[kEvChol], s));
  return SK_OK;
}

// ---- D. back-substitution of the points, and the strategy's vectors behind it (counted with the back-substitution) ----
int BalSolver::enqueue_point_backsub(bool graph) {
  hipStream_t s = stream_;
  // whose cameras' steps this rank accounts for in |step|^2: all, or (segmented) its segment's, + the separator's on the head's rank
  int lo = 0, hi = 9 * C_, lo2 = 0, hi2 = 0;
  if (segmented_) {
    lo = 9 * my_lo_; hi = 9 * my_hi_;
    if (role_ == 0) { lo2 = 9 * cam_b_; hi2 = 9 * C_; }
  }
  launch_bal_backsub(d_, b_scal_.p + kStepSqCam, lo, hi, lo2, hi2, s);  // (and |delta_p|^2 to kStepSqPt)
  if (dogleg()) {  // the two vectors of this Jacobian and their eight scalars
    kt_.begin("dogleg_vector_norms", s); launch_dogleg_vector_norms(d_, dl_, s); kt_.end("dogleg_vector_norms", s);
    kt_.begin("bal_dogleg_products", s); launch_bal_dogleg_products(d_, dl_, s); kt_.end("bal_dogleg_products", s);
    launch_dogleg_reduce_scalars(dl_, s);
    SK_HIP_TRY(hipMemcpyAsync(h_scal_ + kDogleg + kDlScalars, dl_.scal + kDlScalars, (kDlStepSq - kDlScalars) * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  if (bounded_) {  // g . delta and max |delta_j| of the unconstrained step; the candidate becomes P(x + delta)
    kt_.begin("bal_directional_derivative", s); launch_bal_directional_derivative(d_, bd_, s); kt_.end("bal_directional_derivative", s);
    kt_.begin("bal_bounded_candidate", s); launch_bal_bounded_candidate(d_, bd_, 1.0, s); kt_.end("bal_bounded_candidate", s);
    SK_HIP_TRY(hipMemcpyAsync(h_scal_ + kBounds + kBdStepSq, bd_.scal + kBdStepSq, (kBdMaxDelta + 1 - kBdStepSq) * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  if (!graph) SK_HIP_TRY(hipEventRecord(ev_[kEvBacksub], s));
  return SK_OK;
}

// The cost of the point in xc_new / xp_new: the cost kernel (or the tape's), the host-evaluated blocks, the reduction of `rows` rows of
// partial sums to kCandSumSq (and kModel).
int BalSolver::enqueue_candidate_cost(int rows, bool* failed) {
  hipStream_t s = stream_;
  kt_.begin("bal_eval_cost", s);
  if (tape_mode_) launch_bal_eval_cost_tape(d_, tape_dev_, s); else launch_bal_eval_cost(d_, s);
  kt_.end("bal_eval_cost", s);
  int nb_cost = bal_partial_blocks(N_);
  if (d_.num_host > 0) {
    int rc = host_callbacks(d_.xc_new, false, failed);
    if (rc) return rc;
    nb_cost += launch_bal_host_cost(d_, nb_cost, s);
  }
  launch_final_reduce(b_partial_.p, partial_stride_, nb_cost, rows, 0, b_scal_.p + kCandSumSq, s);
  return SK_OK;
}

// What the two trials share behind the launch that formed their candidate (since kEvBegin): its cost — the model term of the cost kernel
// is not used here — the copies of the sum and of the candidate's |x - x_new|^2 (a device scalar of the strategy, to its pinned mirror),
// the one synchronisation, phases 3 and 4.  One device, no host-evaluated blocks (setup(), refuses_bounds()).
int BalSolver::trial_cost(const double* step_sq_dev, int step_sq_slot, double* cost, double* step_norm) {
  hipStream_t s = stream_;
  SK_HIP_TRY(hipEventRecord(ev_[kEvBacksub], s));
  bool failed = false;
  int rc = enqueue_candidate_cost(1, &failed);
  if (rc) return rc;
  SK_HIP_TRY(hipEventRecord(ev_[kEvCost], s));
  SK_HIP_TRY(hipMemcpyAsync(h_scal_ + kCandSumSq, b_scal_.p + kCandSumSq, sizeof(double), hipMemcpyDeviceToHost, s));
  SK_HIP_TRY(hipMemcpyAsync(h_scal_ + step_sq_slot, step_sq_dev, sizeof(double), hipMemcpyDeviceToHost, s));
  SK_HIP_TRY(hipStreamSynchronize(s));
  add_phases(3, 4);
  *cost = failed ? std::numeric_limits<double>::max() : 0.5 * h_scal_[kCandSumSq];  // (as the LM path; no host-evaluated block reaches a trial today)
  *step_norm = std::sqrt(h_scal_[step_sq_slot]);
  return SK_OK;
}

// Parameter bounds (common.hpp: namespace bounds): the candidate P(x + alpha delta) of the line search.
int BalSolver::bounded_trial(double alpha, double* cost, double* step_norm) {
  SK_HIP_TRY(hipEventRecord(ev_[kEvBegin], stream_));
  kt_.begin("bal_bounded_candidate", stream_); launch_bal_bounded_candidate(d_, bd_, alpha, stream_); kt_.end("bal_bounded_candidate", stream_);
  return trial_cost(bd_.scal + kBdStepSq, kBounds + kBdStepSq, cost, step_norm);
}

// DOGLEG (common.hpp: namespace dogleg): the candidate x + (a s + b g) scale from the two vectors on the device.
int BalSolver::dogleg_trial(double a, double b, double* cost, double* step_norm) {
  SK_HIP_TRY(hipEventRecord(ev_[kEvBegin], stream_));
  kt_.begin("bal_dogleg_combine", stream_); launch_bal_dogleg_combine(d_, dl_, a, b, stream_); kt_.end("bal_dogleg_combine", stream_);
  return trial_cost(dl_.scal + kDlStepSq, kDogleg + kDlStepSq, cost, step_norm);
}

// End the capture on `s` and instantiate what was captured.  A runtime that cannot capture this sequence switches the
// replay off for good (graph_mode_ = false; the caller then enqueues the launches directly), with one line on stderr.
int BalSolver::finish_capture(hipStream_t s, hipGraphExec_t* exec) {
  hipGraph_t g = nullptr;
  hipError_t e = hipStreamEndCapture(s, &g);
  if (e == hipSuccess && g) e = hipGraphInstantiate(exec, g, nullptr, nullptr, 0);
  if (g) (void)hipGraphDestroy(g);
  if (e != hipSuccess || !*exec) {
    (void)hipGetLastError();
    *exec = nullptr;
    graph_mode_ = false;
    std::fprintf(stderr, "[skeres_amd] hipGraph capture of the iteration failed (%s): launches are enqueued one by one\n", hipGetErrorString(e));
  }
  return SK_OK;
}

// The reference's director upcall (ceres.i:48; CORE/AutodiffCostFunction.scala:74-78) for the residual blocks whose cost
// function has no device body: parameters down to the host, the caller's Evaluate once per block with the exact native
// signature (jacobians == nullptr on the cost-only branch), the rows back up.  Slow by construction — one PCIe round
// trip per evaluation and host arithmetic — but any generic (9, 3) -> 2 functor can enter DENSE_SCHUR this way.
int BalSolver::host_callbacks(const double* x_dev, bool jac, bool* failed) {
  *failed = false;
  const size_t nc = 9 * (size_t)C_, np = 3 * (size_t)P_;
  SK_HIP_TRY(hipMemcpyAsync(host_x_.data(), x_dev, (nc + np) * sizeof(double), hipMemcpyDeviceToHost, stream_));
  SK_HIP_TRY(hipStreamSynchronize(stream_));
  for (size_t h = 0; h < host_obs_.size(); ++h) {
    const int o = host_obs_[h];
    const CostFunction* cf = host_cf_[h];
    const double* params[2] = {&host_x_[9 * (size_t)h_cam_[o]], &host_x_[nc + 3 * (size_t)h_pt_[o]]};
    double* row = &host_rows_h_[h * (size_t)kHostRow];
    for (int k = 0; k < kHostRow; ++k) row[k] = 0.0;
    if (res_size_ == 2 && cam_size_ == 9 && pt_size_ == 3) {
      double* jptr[2] = {row + 2, row + 20};
      if (!cf->callback(cf->user, params, row, jac ? jptr : nullptr)) { *failed = true; return SK_OK; }
    } else {
      // a smaller shape: the caller's Evaluate writes r residuals and row-major r x c / r x q blocks (CORE/AutodiffCostFunction.scala:115-130);
      // they go into the (2; 9, 3) row the kernels read, the rest of it zero
      double res[2] = {0.0, 0.0}, jc[2 * 9], jq[2 * 3];
      double* jptr[2] = {jc, jq};
      if (!cf->callback(cf->user, params, res, jac ? jptr : nullptr)) { *failed = true; return SK_OK; }
      for (int r = 0; r < res_size_; ++r) {
        row[r] = res[r];
        if (jac) {
          for (int k = 0; k < cam_size_; ++k) row[2 + 9 * r + k] = jc[r * cam_size_ + k];
          for (int k = 0; k < pt_size_; ++k) row[20 + 3 * r + k] = jq[r * pt_size_ + k];
        }
      }
    }
  }
  SK_HIP_TRY(hipMemcpyAsync(b_host_rows_.p, host_rows_h_.data(), host_rows_h_.size() * sizeof(double), hipMemcpyHostToDevice, stream_));
  SK_HIP_TRY(hipStreamSynchronize(stream_));  // (host_rows_h_ is pageable and reused by the next evaluation)
  return SK_OK;
}

int BalSolver::write_back() {
  const size_t nc = 9 * (size_t)C_, np = 3 * (size_t)P_;
  std::vector<double> x(nc + np);
  SK_HIP_TRY(hipMemcpyAsync(x.data(), d_.xc, (nc + np) * sizeof(double), hipMemcpyDeviceToHost, stream_));
  SK_HIP_TRY(hipStreamSynchronize(stream_));
  if (segmented_) {
    // a rank's cameras of the OTHER segment were never updated: every camera from the rank that owns it (the separator's
    // from rank 0; replicas add zeros), summed into a zero-filled table
    std::vector<double> cams(nc, 0.0);
    if (!replica_) {
      const size_t lo = 9 * (size_t)my_lo_, hi = 9 * (size_t)my_hi_;
      std::memcpy(&cams[lo], &x[lo], (hi - lo) * sizeof(double));
      if (role_ == 0) std::memcpy(&cams[9 * (size_t)cam_b_], &x[9 * (size_t)cam_b_], (nc - 9 * (size_t)cam_b_) * sizeof(double));
    }
    DevBuf<double> tmpc;
    SK_HIP_TRY(tmpc.upload(cams, stream_));
    int rc = allreduce(tmpc.p, cams.size());
    if (rc) return rc;
    SK_HIP_TRY(hipMemcpyAsync(x.data(), tmpc.p, nc * sizeof(double), hipMemcpyDeviceToHost, stream_));
    SK_HIP_TRY(hipStreamSynchronize(stream_));
  }
  for (int i = 0; i < C_; ++i) if (cam_block_[i] >= 0) std::memcpy(problem_->block_ptr[cam_block_[i]], &x[9 * (size_t)i], cam_size_ * sizeof(double));
  if (!opt_.allreduce) {
    for (int q = 0; q < P_; ++q) std::memcpy(problem_->block_ptr[pt_block_[local_pt_[q]]], &x[nc + 3 * (size_t)q], pt_size_ * sizeof(double));
    return SK_OK;
  }
  // every rank returns ALL points: zero-filled table, own slice filled, sum-reduced
  std::vector<double> all(3 * (size_t)P_total_, 0.0);
  if (!replica_)  // (a replica adds zeros; so does a copy of a retained point whose home is another rank: the copies come last)
    for (int q = 0; q < P_own_; ++q) std::memcpy(&all[3 * (size_t)local_pt_[q]], &x[nc + 3 * (size_t)q], 3 * sizeof(double));
  DevBuf<double> tmp;
  SK_HIP_TRY(tmp.upload(all, stream_));
  int rc = allreduce(tmp.p, all.size());
  if (rc) return rc;
  SK_HIP_TRY(hipMemcpyAsync(all.data(), tmp.p, all.size() * sizeof(double), hipMemcpyDeviceToHost, stream_));
  SK_HIP_TRY(hipStreamSynchronize(stream_));
  for (int q = 0; q < P_total_; ++q) std::memcpy(problem_->block_ptr[pt_block_[q]], &all[3 * (size_t)q], pt_size_ * sizeof(double));
  return SK_OK;
}

}  // namespace

std::unique_ptr<SolverBase> make_bal_solver(const Options& o, Problem* p) { return std::unique_ptr<SolverBase>(new BalSolver(o, p)); }

}  // namespace sk
