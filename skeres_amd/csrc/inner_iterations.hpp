// Inner iterations on the device (Solver::Options::use_inner_iterations): after a trust-region step every parameter block of an
// independent set is minimised on its own, the others held, then the next set follows (plan: inner_plan.hpp; kernels:
// inner_kernels.hip; constants: common.hpp, namespace inner).
//
// The component owns nothing of the problem's image: it is handed the solver's DeviceJacobian, its values array with the index
// arrays, its residual-only staging and its residual and cost-term arrays, and refines a point in Problem::Evaluate's layout in
// place.  It leaves the values array UNSCALED at whatever point its last round evaluated, and the residual and cost-term arrays
// with it: the caller evaluates again before it reads any of them.
//
// Rounds.  The blocks of a group share no residual block, so one ROUND advances every block of the group that is still running
// by one Levenberg-Marquardt iteration, and the result is what the blocks solved one after the other would give:
//   1. the whole-problem evaluation with the Jacobian at x (the existing launches);
//   2. per block g = J_b^T r (launch_cgnr_jtw), H = J_b^T J_b (launch_cgnr_block_diag), the sum of its cost terms;
//   3. inner_step_kernel: tests, scaling, D, Cholesky, the step, the model, the candidate through Plus into a second point;
//   4. the residual-only evaluation at the second point;  5. the candidates' costs, inner_accept_kernel, the count of running blocks.
// The host enqueues inner::kBatch rounds and reads the flags back; every kernel of a round returns at once when the group is done
// and (steps 3 to 5) for a block that is done, so a refinement returns the same bytes for every batch size.  Ordinary
// stream-ordered launches: no graph, no second stream, no kernel waits for another.
#pragma once
#include <vector>

#include "inner_kernels.hpp"
#include "inner_plan.hpp"
#include "jacobian_device.hpp"

namespace sk {

class InnerIterations {
 public:
  struct Shared {
    DeviceJacobian* dj = nullptr;
    CgnrJac jac{};                                          // the values array and the index arrays of both plans
    const std::vector<size_t>* group_stage_cost = nullptr;  // the residual-only staging: per group, and on the device per block
    const size_t* blk_stage_cost = nullptr;
    double* r = nullptr; double* rc = nullptr; double* cterm = nullptr; double* cterm_c = nullptr;  // at x, at the second point
    double* jtw_partial = nullptr; double* bd_partial = nullptr;  // the partial sums of the full plan's long blocks: a group has no more
    int num_cols = 0, num_ambient = 0, num_pb = 0;
    size_t matrix_entries = 0;
  };
  ~InnerIterations();
  int setup(const InnerPlan& plan, const Shared& shared, hipStream_t s);
  // x_dev is refined in place; *rounds: the rounds of all groups.  Synchronises the stream.
  int refine(double* x_dev, int* rounds);
  // per parameter block the iterations and the inner::Status of its solve in the last refinement (-1: not refined)
  int blocks(int* iterations, int* status);
  int num_groups() const { return (int)groups_.size(); }

 private:
  struct Group {
    DevBuf<int> b[10], pb, cost_rb;
    InnerGroupDev dev{};
  };
  int round(const Group& G, double* x_dev);

  Shared sh_;
  hipStream_t s_ = nullptr;
  std::vector<Group*> groups_;
  std::vector<int> refined_pb_;   // per parameter block: 1 when a group holds it
  bool refined_once_ = false;
  DevBuf<double> b_xc_, b_st_, b_scale_, b_g_, b_H_, b_csum_, b_csum_c_, b_cost_partial_;
  DevBuf<int> b_sti_, b_flags_;
  InnerDev dev_{};
  int* h_flags_ = nullptr;
};

}  // namespace sk
