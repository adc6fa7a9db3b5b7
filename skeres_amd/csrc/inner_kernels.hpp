// Launchers of inner_kernels.hip: the device side of the inner iterations (plan: inner_plan.hpp; host: inner_iterations.hip).
// fp64, wave64, every sum in an order the plan fixes, no floating-point atomics.  The gradient J_b^T r and the sums J_b^T J_b of
// a group's blocks are cgnr_kernels.hpp's launch_cgnr_jtw (kCgnrJtwPlain) and launch_cgnr_block_diag on the group's lists.
#pragma once
#include <hip/hip_runtime.h>

#include "cgnr_kernels.hpp"
#include "common.hpp"

namespace sk {

// The flags of a group's rounds (ints).  kInDone sits where kCgDone does, so that the CGNR launches take the same array.
enum InnerFlag { kInRounds = 0, kInDone = 1, kInActive = 2, kInFlagCount = 4 };
static_assert((int)kInDone == (int)kCgDone, "launch_cgnr_jtw and launch_cgnr_block_diag read the group's done flag");

// Per parameter block, the state of its solve: doubles at st[pb * kInDCount + .], ints at sti[pb * kInICount + .]
enum InnerD { kInRadius = 0, kInDecrease, kInCost, kInModel, kInStepNorm, kInXNorm, kInDCount };
enum InnerI { kInStatus = 0, kInIters, kInInvalid, kInTried, kInScaled, kInICount };

// A group on the device: its blocks as a cols-style list, per block the parameter block, per slot-list entry the residual block
// whose cost term it adds (-1: none)
struct InnerGroupDev {
  CgnrCols cols;
  const int* pb;
  const int* cost_rb;
};
// The buffers of the component.  g [tangent columns] and H [the plan's matrix entries] in the full plan's places; csum, csum_c
// [blocks of the largest group]: the sums of the blocks' cost terms at x and at the candidate
struct InnerDev {
  double* st; int* sti;
  double* scale;   // [tangent columns] the block's Jacobi scaling, from its first Jacobian
  double* g; double* H;
  double* csum; double* csum_c;
  double* cost_partial;  // [partial sums of the largest group * kCgnrLanes]
  int* flags;
};

// every block of the group starts: running, radius and decrease factor at their initial values; the flags are zeroed
void launch_inner_begin(const InnerGroupDev& G, const InnerDev& D, hipStream_t s);
// out[e] = sum of the cost terms of block e's residual blocks, by the parts of its slot list (kCgnrLanes lanes per part, a
// butterfly, a second launch for long blocks)
void launch_inner_cost(const InnerGroupDev& G, const InnerDev& D, const double* cterm, double* out, hipStream_t s);
// one lane per block: tests, scaling, D, Cholesky, the step, its model, the candidate into xc
void launch_inner_step(const InnerGroupDev& G, const InnerDev& D, const ParamBlock* pblocks, const double* x, double* xc, hipStream_t s);
// one lane per block: tolerance tests, rho, accept (xc -> x) or reject (x -> xc), radius; counts the blocks still running
void launch_inner_accept(const InnerGroupDev& G, const InnerDev& D, const ParamBlock* pblocks, double* x, double* xc, hipStream_t s);
// one lane: the round is counted, the group is done when no block is running
void launch_inner_round_end(const InnerDev& D, hipStream_t s);
// partials[chunk] = sum (a_i - b_i)^2 over chunks of kCgnrDotChunk
void launch_inner_diff_sq(const double* a, const double* b, int n, double* partials, hipStream_t s);

}  // namespace sk
