// Launchers of evaluate_kernels.hip: Problem::Evaluate on the device (plan: evaluate_plan.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"

namespace sk {

// One evaluation group: lane l evaluates residual block blocks[members[l]] of the problem and writes entry e of its
// results to stage[e * count + l] (e = r: residual r; num_residuals + r * dim + k: dJ_r / dparameter_k).
struct EvaluateEvalArgs {
  int count;
  const int* members;       // [count] positions in the list of residual blocks
  const int* blocks;        // the list: residual block of the problem per position
  const double* consts;     // the problem's constants ...
  const size_t* const_off;  // ... and where each residual block's begin
  const int* xoff;          // offset in x of the parameter block of every (residual block, slot) of the problem
  const size_t* pidx_off;   // [residual blocks + 1]
  const double* x;          // every parameter block of the problem, one after the other
  double* stage;            // the group's staging
  int* fail_flag;
};

struct EvaluateFinishArgs {
  int num_blocks;             // listed residual blocks
  const size_t* blk_stage;    // per listed block: first staging entry of its lane, the stride between entries,
  const int* blk_stride;
  const int* blk_dim;         // the functor's number of parameters,
  const int* blk_loss;        // the root of its loss (-1: none, or not applied),
  const int* row_off;         // its first row [num_blocks + 1], its first value [num_blocks + 1], its slots [num_blocks + 1]
  const int* val_off;
  const int* slot_begin;
  const int* slot_block;      // per slot: parameter block, first parameter inside the functor, first value inside a row (-1: none)
  const int* slot_k0;
  const int* slot_pos;
  const ParamBlock* pblocks;  // per parameter block of the problem (global_off: in x; local_size: the tangent size)
  const LossNode* nodes;
  const double* x;
  const double* stage;
  double* residuals;          // [rows], corrected
  double* values;             // [non-zeros]; null: residuals and cost terms only
  double* cterm;              // [num_blocks] rho(|r|^2) (|r|^2 without a loss)
};

struct EvaluateGradientArgs {
  int num_column_blocks;
  const int* grad_col;    // first column, tangent size
  const int* grad_size;
  const int* grad_begin;  // [num_column_blocks + 1] into grad_slots
  const int* grad_slots;
  const int* slot_owner;
  const int* slot_pos;
  const int* row_off;
  const int* val_off;
  const double* residuals;
  const double* values;
  double* gradient;
};

constexpr int kEvaluateSumChunk = 4096;  // cost terms per first-stage workgroup of the cost sum

void launch_evaluate_eval(int functor_id, bool jac, const EvaluateEvalArgs& a, hipStream_t s);
// false: the tape's register file does not fit the LDS (nothing was launched)
bool launch_evaluate_eval_tape(const TapeDevBuffers& tb, bool jac, const EvaluateEvalArgs& a, hipStream_t s);
void launch_evaluate_finish(const EvaluateFinishArgs& a, hipStream_t s);
void launch_evaluate_gradient(const EvaluateGradientArgs& a, hipStream_t s);
// *cost = 1/2 sum cterm, in a fixed order; partials: at least ceil(n / kEvaluateSumChunk) doubles
void launch_evaluate_cost(const double* cterm, int n, double* partials, double* cost, hipStream_t s);

// sk_problem_evaluate (evaluate.hip).  Every output may be null.  launch_seconds (may be null): device seconds of the call's
// phases from HIP events on its stream — 0 uploads, 1 evaluation launches (with the host callbacks), 2 finish, 3 gradient, 4 cost,
// 5 downloads.
struct EvaluateOptions;
constexpr int kEvaluatePhases = 6;
int problem_evaluate(const Problem& p, const EvaluateOptions* options, double* cost, double* residuals, double* gradient, double* values,
                     double* launch_seconds);

}  // namespace sk
