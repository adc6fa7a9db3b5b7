// Host plan of Problem::Evaluate (sk_problem_evaluate): rows, columns, where every Jacobian block goes, the evaluation groups
// and the summation order of the gradient — plain C++ over a Problem, compiled without the device headers like bal_plan.cpp.
//
// Conventions (Ceres 1.x's Problem::Evaluate, restated from memory — include/skeres_amd.h):
//   rows     the residual blocks of the list in list order (no list: in the order added), num_residuals rows each;
//   columns  the parameter blocks of the list in list order (no list: in the order first seen), each with its TANGENT size
//            (the local size of its parameterization, else its size); a block absent from a given list has no columns; a
//            constant block that is listed keeps its columns and has no stored entries — unlike the solvers, which give a
//            constant block local size 0;
//   values   per residual block and stored parameter block the dense num_residuals x tangent size block, zeros included, the
//            blocks of a row in ascending column order.
// The values of the listed residual blocks follow one another in values[]: block i owns values[val_off[i], val_off[i + 1]),
// row-major num_residuals x (its row width).
#pragma once
#include <string>
#include <vector>

#include "problem.hpp"

namespace sk {

struct EvaluateOptions {  // ceres::Problem::EvaluateOptions (num_threads: ignored)
  bool apply_loss_function = true;
  std::vector<int> residual_blocks;       // empty: all, in the order added
  std::vector<double*> parameter_blocks;  // empty: all, in the order first seen
  int device = -1;                        // -1: the current device
};

// The residual blocks of one functor (or of one tape), one lane each; a host-callback block is a group of its own.  The group's
// staging is PLANES: entry e of lane l at stage_off + e * count + l, e = r for the residuals and num_residuals + r * dim + k for
// dJ_r / dparameter_k (k numbered through the functor's parameter blocks), so that a wave's stores are contiguous.
struct EvaluateGroup {
  int functor = 0;          // sk_functor_id, or kTapeFunctorBase + tape
  int num_residuals = 0, dim = 0;
  std::vector<int> members; // positions in EvaluatePlan::blocks, ascending
  size_t stage_off = 0;
};

struct EvaluatePlan {
  int num_rows = 0, num_cols = 0;
  long long num_nonzeros = 0;
  std::vector<int> col_off, col_size;  // per parameter block of the problem: first column (-1: no columns), tangent size
  std::vector<int> blocks;             // the listed residual blocks
  std::vector<int> row_off, val_off;   // [blocks + 1]
  // per (listed block, parameter slot): slots of block i are [slot_begin[i], slot_begin[i + 1])
  std::vector<int> slot_begin;
  std::vector<int> slot_block;  // parameter block of the problem
  std::vector<int> slot_k0;     // its first parameter inside the functor's flattened parameters
  std::vector<int> slot_pos;    // first value of the slot inside a row of its residual block; -1: nothing stored (absent or constant)
  std::vector<int> slot_owner;  // its listed block
  std::vector<EvaluateGroup> groups;  // device functors by id, then tapes, then the host-callback blocks in list order
  std::vector<size_t> blk_stage;      // per listed block: its lane's first staging entry ...
  std::vector<int> blk_stride;        // ... and the stride between entries (the group's count)
  size_t stage_size = 0, callback_stage_begin = 0;  // host-callback groups lie in [callback_stage_begin, stage_size)
  // gradient: column block c covers columns [grad_col[c], grad_col[c] + grad_size[c]) and sums the slots
  // grad_slots[grad_begin[c] .. grad_begin[c + 1]) in that order — list (row) order
  std::vector<int> grad_col, grad_size, grad_begin, grad_slots;
  std::vector<int> rows, cols;  // the CRS structure (only when asked for)
};

// Returns an sk_status; *why says what is wrong.  structure: fill rows / cols; gradient: fill the grad_* lists; jacobian: the
// staging holds the Jacobian planes too (else the num_residuals residual planes of every group alone).
int evaluate_plan_build(const Problem& p, const EvaluateOptions* options, bool structure, bool gradient, bool jacobian, EvaluatePlan* plan,
                        std::string* why);
// The staging of the plan's groups, as evaluate_plan_build lays it out for `jacobian`: per group its stage_off, per listed block
// its blk_stage (and its blk_stride, where asked for); returns the stage_size.  With jacobian == false on a plan built with the
// Jacobian planes: where a residual-only evaluation of the same groups puts its results (blk_stride is the same).
size_t evaluate_plan_staging(const EvaluatePlan& plan, bool jacobian, std::vector<size_t>* group_stage, std::vector<size_t>* blk_stage,
                             std::vector<int>* blk_stride = nullptr);

}  // namespace sk
