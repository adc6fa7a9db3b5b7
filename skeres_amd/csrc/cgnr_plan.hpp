// Host plan of the CGNR solver (cgnr_solver.hip): the block-sparse Jacobian's layout is Problem::Evaluate's (evaluate_plan.hpp) over
// every residual block and every parameter block; this plan adds what the two products J p and J^T w, the block sums and the
// preconditioner read — plain C++ over a Problem, compiled without the device headers like bal_plan.cpp and evaluate_plan.cpp.
//
// Columns.  The tangent vector of the solver holds the parameter blocks that move, in problem order, each with its tangent size;
// a constant block and a block whose tangent size is 0 have no columns here (Problem::Evaluate keeps a constant block's columns;
// its values array has no entries for them either way, so the values layout is shared).
//
// Summation order.  Column block c sums over the slots cb_slots[cb_begin[c] .. cb_begin[c + 1]) — the stored (residual block,
// parameter slot) pairs on that block, ascending with the rows.  The list is cut into PARTS of cgnr::kPartSlots (64) slots, the
// last one shorter; a part is summed by kCgnrLanes lanes (lane l takes the part's slots l, l + kCgnrLanes, ..., then a butterfly
// over the lanes), and a block of more than one part (a LONG block: a camera, a shared calibration block) sums its parts the same
// way in a second launch: lane l takes parts l, l + kCgnrLanes, ...  Parts and their order are fixed here, so the sum of a block
// depends on the problem alone, never on a grid size, and no launch uses a floating-point atomic.
#pragma once
#include <string>
#include <vector>

#include "evaluate_plan.hpp"

namespace sk {

constexpr int kCgnrMaxBlock = 16;   // largest tangent size of a parameter block (the preconditioner's Cholesky lives in one thread)
constexpr int kCgnrPartSlots = 64;  // == cgnr::kPartSlots (common.hpp; static_assert in cgnr_solver.hip)

struct CgnrPlan {
  EvaluatePlan eval;                   // staging sized for residuals + Jacobian planes
  std::vector<size_t> blk_stage_cost;  // per residual block: its lane's first staging entry in a residual-only evaluation ...
  std::vector<size_t> group_stage_cost;  // ... and per evaluation group its staging offset
  int num_cols = 0, num_ambient = 0;   // tangent size of the problem, size of x
  std::vector<int> block_off;          // [parameter blocks + 1] in x
  std::vector<int> pb_type, pb_local_size, pb_local_off;  // per parameter block: ParameterizationType (kParamConstant for constant blocks), tangent size and first column (0 / -1: none)
  std::vector<unsigned> pb_mask;
  std::vector<int> slot_col, slot_size;  // per slot of eval: first column and tangent size (-1 / 0 where nothing is stored)
  std::vector<int> row_block;            // per row: its residual block
  // column blocks (the parameter blocks that move)
  std::vector<int> cb_col, cb_size, cb_block;  // first column, tangent size, parameter block of the problem
  std::vector<int> cb_moff;                    // [column blocks + 1] first entry of the block's size x size matrix (block sums, factors)
  std::vector<int> cb_begin, cb_slots;         // [column blocks + 1]; slots in row order
  // parts of the slot lists, in column-block order
  std::vector<int> part_cb, part_begin, part_end;  // column block; the part's range of cb_slots
  std::vector<int> part_out;                       // -1: the block's only part; else the index of its partial sum
  std::vector<int> long_cb, long_begin;            // long blocks; [long blocks + 1] their ranges of partial sums
  int num_partials = 0;
};

// "" when CGNR takes the problem, else why not (SK_ERR_UNSUPPORTED).  Host-callback blocks, a tangent size above kCgnrMaxBlock,
// DOGLEG, parameter bounds, more than one rank, dense rows.
std::string cgnr_refusal(const Problem& p, int world, bool dogleg);
// Returns an sk_status; *why says what is wrong.
int cgnr_plan_build(const Problem& p, CgnrPlan* plan, std::string* why);

}  // namespace sk
