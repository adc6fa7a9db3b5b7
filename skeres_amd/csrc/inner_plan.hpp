// Host plan of the inner iterations (Solver::Options::use_inner_iterations; device side: inner_iterations.hip): the groups of
// parameter blocks that are refined after every trust-region step — plain C++ over a Problem and a CgnrPlan, compiled without
// the device headers like cgnr_plan.cpp.
//
// Groups.  Group 0, 1, ... are each an independent set of moving column blocks of the CGNR plan: two blocks are neighbours when
// a residual block names both.  Automatic: group 0 is jacobian_plan.hpp's greedy_independent_set on the moving blocks, group k
// the same function on the blocks still ungrouped, their neighbours counted among the ungrouped blocks alone, until none is
// left (a bundle-adjustment problem: the points, then the cameras).  Given by the caller (sk_options_set_inner_iteration_ordering):
// block pointers with a group id each; unlisted blocks are not refined, constant blocks are ignored, the ids are compressed
// to 0, 1, ... in ascending order.
//
// Per group the blocks are a cols-style list of their own (cgnr_plan.hpp: CgnrColumnSubset), columns and matrix offsets the
// full plan's, the slot lists cut into parts of kCgnrPartSlots, so that cgnr_jtw_kernel and cgnr_block_diag_kernel take the
// list as it is.  A block's cost is summed over the same list and the same parts: cost_rb names, per entry of cb_slots, the
// residual block whose cost term the entry adds, or -1 where the residual block names the parameter block a second time.
#pragma once
#include <string>
#include <vector>

#include "cgnr_plan.hpp"

namespace sk {

struct InnerGroup {
  CgnrColumnSubset blocks;    // cb: column blocks of the CGNR plan's cols, ascending
  std::vector<int> pb;        // per block of the group: its parameter block
  std::vector<int> cost_rb;   // per entry of blocks.cb_slots: the residual block, or -1 (see above)
};

struct InnerPlan {
  std::vector<int> group_of_cb;  // per column block: its group, -1 not refined
  std::vector<InnerGroup> groups;
  int max_group_blocks = 0, max_partials = 0;
};

// "" when inner iterations run under this linear solver type, else why not (SK_ERR_UNSUPPORTED), naming it: from the options alone.
std::string inner_refusal(int linear_solver_type, const char* name);
// blocks / groups: the caller's ordering (both empty: automatic).  Returns an sk_status; *why says what is wrong — an unknown
// block, a negative group, two neighbours in one group (SK_ERR_INVALID_ARGUMENT).
int inner_plan_build(const Problem& p, const CgnrPlan& C, const std::vector<double*>& blocks, const std::vector<int>& groups, InnerPlan* plan, std::string* why);

}  // namespace sk
