// Host plan of the CGNR solver (cgnr_solver.hip): the block-sparse Jacobian's layout is Problem::Evaluate's (evaluate_plan.hpp) over
// every residual block and every parameter block; this plan adds what the two products J p and J^T w, the block sums and the
// preconditioner read — plain C++ over a Problem, compiled without the device headers like bal_plan.cpp and evaluate_plan.cpp.
//
// Columns: jacobian_plan.hpp's TangentColumns, a constant block counted with tangent size 0.
//
// Summation order.  Column block c sums over the slots cb_slots[cb_begin[c] .. cb_begin[c + 1]) — the stored (residual block,
// parameter slot) pairs on that block, ascending with the rows.  The list is cut into PARTS of cgnr::kPartSlots (64) slots, the
// last one shorter; a part is summed by kCgnrLanes lanes (lane l takes the part's slots l, l + kCgnrLanes, ..., then a butterfly
// over the lanes), and a block of more than one part (a LONG block: a camera, a shared calibration block) sums its parts the same
// way in a second launch: lane l takes parts l, l + kCgnrLanes, ...  Parts and their order are fixed here (jacobian_plan.hpp:
// cut_parts), so the sum of a block depends on the problem alone, never on a grid size, and no launch uses a floating-point atomic.
#pragma once
#include <string>
#include <vector>

#include "evaluate_plan.hpp"
#include "jacobian_plan.hpp"

namespace sk {

constexpr int kCgnrMaxBlock = 16;   // largest tangent size of a parameter block (the preconditioner's Cholesky lives in one thread)

struct CgnrPlan {
  EvaluatePlan eval;                   // staging sized for residuals + Jacobian planes
  std::vector<size_t> blk_stage_cost;  // per residual block: its lane's first staging entry in a residual-only evaluation ...
  std::vector<size_t> group_stage_cost;  // ... and per evaluation group its staging offset
  TangentColumns cols;                 // the parameter blocks that move; a constant block has tangent size 0 and first column -1
  std::vector<int> slot_col, slot_size;  // per slot of eval: first column and tangent size (-1 / 0 where nothing is stored)
  std::vector<int> row_block;            // per row: its residual block
  // per column block of cols
  std::vector<int> cb_moff;             // [column blocks + 1] first entry of the block's size x size matrix (block sums, factors)
  std::vector<int> cb_begin, cb_slots;  // [column blocks + 1]; slots in row order
  PartList parts;                       // of the slot lists cb_slots[cb_begin[c] .. cb_begin[c + 1]), in column-block order
};

// "" when CGNR takes the problem, else why not (SK_ERR_UNSUPPORTED).  Host-callback blocks, a tangent size above kCgnrMaxBlock,
// DOGLEG, parameter bounds, more than one rank, dense rows.
std::string cgnr_refusal(const Problem& p, int world, bool dogleg);
// Returns an sk_status; *why says what is wrong.
int cgnr_plan_build(const Problem& p, CgnrPlan* plan, std::string* why);

}  // namespace sk
