// The device image of a Problem and its EvaluatePlan, and the launches that fill Problem::Evaluate's values array from it: what
// sk_problem_evaluate (evaluate.hip), the CGNR solver (cgnr_solver.hip) and sk_covariance_compute (covariance.hip) share.
// Kernels: evaluate_kernels.hip.
#pragma once
#include <map>
#include <vector>

#include "evaluate_kernels.hpp"
#include "evaluate_plan.hpp"
#include "jacobian_plan.hpp"

namespace sk {

// device time between marks on the stream; off: mark() does nothing and every time is 0
struct Marks {
  hipStream_t s = nullptr;
  bool on = true;
  std::vector<hipEvent_t> ev;
  void mark() { if (!on) return; hipEvent_t e; if (hipEventCreate(&e) == hipSuccess) { (void)hipEventRecord(e, s); ev.push_back(e); } }
  double seconds(size_t i) const {  // between marks i and i + 1, once the stream has passed them
    float ms = 0.f;
    return i + 1 < ev.size() && hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess ? 1e-3 * ms : 0.0;
  }
  ~Marks() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
};

// An upload that leaves no null pointer for a kernel argument: an empty list goes up as one zero.
template <class T>
hipError_t upload_padded(DevBuf<T>& d, const std::vector<T>& h, hipStream_t s) {
  static const std::vector<T> zero(1, T(0));
  return d.upload(h.empty() ? zero : h, s);
}

// The ParamBlock of every parameter block of the problem, as the finish kernel, CGNR's candidate kernel and the covariance's lift
// read them; global_size, global_off and constant_mask are the problem's.  The rest by caller:
//                      type                            local_off              local_size
//   T == nullptr       never kParamConstant            P.col_off[b]           P.col_size[b]               (Problem::Evaluate)
//   T of kZero         kParamConstant for constants    -1 for constants       0 for constants             (CGNR)
//   T of kKeep         kParamConstant for constants    -1 for constants       Problem::Evaluate's         (Covariance)
// The values array is the same under all three: the finish kernel reads the blocks of stored slots alone, which are never constant.
std::vector<ParamBlock> param_blocks(const Problem& p, const EvaluatePlan& P, const TangentColumns* T);

class DeviceJacobian {
 public:
  // Host work alone: reads the caller's parameter memory, now, and lays out what upload() sends.  The problem and the plan must
  // outlive this object.  apply_loss: false evaluates every residual block without its loss function.
  void gather(const Problem& p, const EvaluatePlan& P, std::vector<ParamBlock> pblocks, bool apply_loss);
  // The point, the problem and the plan to the device.  want_values: the values array is allocated (the plan was built with the
  // Jacobian planes).  by_column: slot_owner is uploaded, for those who walk the values by column block.
  int upload(bool want_values, bool by_column, hipStream_t s);
  // The tapes of the plan's recorded functors, now (evaluate() uploads a tape at its first use otherwise).
  int upload_tapes();
  // The evaluation launches of one point, a launch per functor / tape into the staging planes; jac: with the Jacobian planes.
  // Host-callback blocks are evaluated on the host at the point that was gathered, and their staging is uploaded.  group_stage:
  // per group its staging offset when it is not the plan's (evaluate_plan_staging: a residual-only evaluation on a plan built
  // with the Jacobian planes; not with host-callback blocks).
  int evaluate(const double* x_dev, bool jac, const std::vector<size_t>* group_stage = nullptr);
  // Loss correction, projection into the tangent space and the scatter into `values`; values == nullptr: residuals and cost terms
  // alone.  blk_stage: the device copy of the per-block staging offsets that go with group_stage (nullptr: the plan's).
  void finish(const double* x_dev, double* residuals, double* values, double* cterm, const size_t* blk_stage = nullptr);

  double* x() const { return x_.p; }            // the gathered point
  double* values() const { return values_.p; }  // [non-zeros]; null without want_values
  const int* row_off() const { return row_off_.p; }
  const int* val_off() const { return val_off_.p; }
  const int* slot_begin() const { return slot_begin_.p; }
  const int* slot_pos() const { return slot_pos_.p; }
  const int* slot_owner() const { return slot_owner_.p; }  // null without by_column
  const ParamBlock* pblocks() const { return pblocks_.p; }
  int* fail_flag() const { return fail_.p; }  // set by a functor that reports failure; zeroed by upload()

 private:
  int tape(int functor, const TapeDevBuffers** tb);

  const Problem* p_ = nullptr;
  const EvaluatePlan* P_ = nullptr;
  hipStream_t s_ = nullptr;
  // what the uploads read on the host: alive as long as the device copies
  std::vector<double> h_x_, h_cb_stage_;
  std::vector<int> h_block_off_, h_xoff_, h_blk_dim_, h_blk_loss_, h_members_;
  std::vector<size_t> member_off_;
  std::vector<ParamBlock> h_pblocks_;
  std::vector<LossNode> h_nodes_;
  std::map<int, TapeDevBuffers> tapes_;
  DevBuf<double> x_, consts_, stage_, values_;
  DevBuf<size_t> const_off_, pidx_off_, blk_stage_;
  DevBuf<int> xoff_, blocks_, members_, blk_stride_, blk_dim_, blk_loss_, row_off_, val_off_, slot_begin_, slot_block_, slot_k0_, slot_pos_, slot_owner_, fail_;
  DevBuf<ParamBlock> pblocks_;
  DevBuf<LossNode> nodes_;
};

}  // namespace sk
