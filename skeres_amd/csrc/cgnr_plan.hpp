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
//
// Schur elimination (sk_options_set_schur_elimination).  E is jacobian_plan.hpp's greedy independent set of the column blocks, F the
// rest.  The vectors keep the columns of the full tangent space (an e-block's entries are zero while the CG loop runs), so F and
// E are each a list of column blocks with slot lists and parts of its own (CgnrColumnSubset) that the launches of the products,
// of the fused update and of the projection are handed in place of the full list.  The block diagonal of S sums, per F block g,
// over g's distinct e-neighbours in ascending order (a PAIR: every residual block that names both, as (slot of g, slot of e) in
// row order); the pair lists are cut into parts of kCgnrPartSlots pairs like the slot lists.
#pragma once
#include <string>
#include <vector>

#include "evaluate_plan.hpp"
#include "jacobian_plan.hpp"

namespace sk {

constexpr int kCgnrMaxBlock = 16;   // largest tangent size of a parameter block (the preconditioner's Cholesky lives in one thread)

// Some column blocks of a plan, ascending, as a cols-style list of their own: columns and matrix offsets are the full plan's
struct CgnrColumnSubset {
  std::vector<int> cb;                          // the column blocks of cols
  std::vector<int> cb_col, cb_size, cb_moff;    // per block of the subset: first column, tangent size, first matrix entry
  std::vector<int> cb_begin, cb_slots;          // [blocks + 1]; slots in row order
  PartList parts;
};

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
  // the Schur elimination; all empty without it
  std::vector<int> cb_elim;             // per column block: 1 in E
  CgnrColumnSubset F, E;
  int reduced_cols = 0;                 // tangent size of F
  std::vector<int> slot_size_f;         // slot_size with 0 on the slots of E: J_F v by the launch of J v
  std::vector<int> fp_begin;            // [F blocks + 1] the pairs of each F block ...
  std::vector<int> fp_e;                // ... per pair the e-block (a column block of cols), ascending inside an F block
  std::vector<int> fp_slot_begin, fp_slot_g, fp_slot_e;  // [pairs + 1]; per term of a pair the slot of g and the slot of e, in row order
  PartList fp_parts;                    // of the pair lists
};

// "" when CGNR takes the problem, else why not (SK_ERR_UNSUPPORTED).  Host-callback blocks, a tangent size above kCgnrMaxBlock,
// DOGLEG, parameter bounds, more than one rank, dense rows.
std::string cgnr_refusal(const Problem& p, int world, bool dogleg);
// Returns an sk_status; *why says what is wrong.
int cgnr_plan_build(const Problem& p, CgnrPlan* plan, std::string* why, bool schur_elimination = false);

}  // namespace sk
