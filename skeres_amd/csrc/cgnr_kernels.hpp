// Launchers of cgnr_kernels.hip: the device side of the CGNR solver (plan: cgnr_plan.hpp; host: cgnr_solver.hip).
// fp64, wave64, every sum in an order the plan fixes, no floating-point atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"

namespace sk {

// The scalars of the solver on the device (one buffer of doubles, copied back in one piece) ...
enum CgnrScal {
  kCgRho = 0, kCgRhoLast, kCgPq, kCgAlpha, kCgBeta, kCgQ0, kCgQ1, kCgZeta, kCgBb,  // conjugate gradients (common.hpp: namespace cgnr)
  kCgModel,                    // (J delta) . (r + J delta / 2) of the step
  kCgStepSq,                   // |x - candidate|^2
  kCgGradMax, kCgXSq,          // after an evaluation: max_j |g_j|, |x|^2
  kCgCost, kCgCandCost,        // 1/2 sum rho at x and at the candidate
  kCgScalCount
};
// ... and its counters and flags (ints).  Every kernel of the CG loop returns at once when kCgDone is set.
enum CgnrFlag { kCgIt = 0, kCgDone, kCgStatus, kCgFail, kCgFlagCount };

// The block-sparse Jacobian: Problem::Evaluate's values array, scaled in place, with the index arrays of both plans.
struct CgnrJac {
  int num_rows;
  const int* row_block;   // [rows]
  const int* row_off;     // [residual blocks + 1]
  const int* val_off;     // [residual blocks + 1]
  const int* slot_begin;  // [residual blocks + 1]
  const int* slot_pos;    // per slot: first value inside a row (-1: nothing stored), first column, tangent size, residual block
  const int* slot_col;
  const int* slot_size;
  const int* slot_owner;
  double* values;
};
// The column blocks, their slot lists and the parts of those lists (cgnr_plan.hpp).
struct CgnrCols {
  int num_cb, num_parts, num_long;
  const int* cb_col; const int* cb_size; const int* cb_moff; const int* cb_slots;
  const int* part_cb; const int* part_begin; const int* part_end; const int* part_out;
  const int* long_cb; const int* long_begin;
};

constexpr int kCgnrLanes = 16;        // lanes that sum one part (and the parts of one long block)
constexpr int kCgnrDotChunk = 4096;   // elements per first-stage workgroup of a dot product
constexpr int kCgnrBlockChunk = 256;  // column blocks per first-stage workgroup of the fused update

// --- after an evaluation -----------------------------------------------------------------------------------------------------------
// bsum[cb_moff[c] + a * size + b] = sum over the block's slots of (J_slot^T J_slot)(a, b); partial: [num_partials * 256]
// flags (may be null): the done flag of whoever enqueues ahead (the inner iterations: inner_iterations.hip)
void launch_cgnr_block_diag(const CgnrJac& J, const CgnrCols& C, double* bsum, double* partial, hipStream_t s, const int* flags = nullptr);
// scale_j = 1 / (1 + sqrt(bsum's diagonal)) — iteration 0, from the sums of the unscaled Jacobian
void launch_cgnr_scale_compute(const CgnrCols& C, const double* bsum, double* scale, hipStream_t s);
// values <- values diag(scale), in place
void launch_cgnr_scale_apply(const CgnrJac& J, const double* scale, hipStream_t s);
// b = -gs, scal[kCgGradMax] = max |gs_j / scale_j|, scal[kCgXSq] = |x|^2 (one workgroup)
void launch_cgnr_gradient_norms(const double* gs, const double* scale, int n, const double* x, int ng, double* b, double* scal, hipStream_t s);

// --- per linear solve --------------------------------------------------------------------------------------------------------------
// D2 = clamp(diag bsum, lo, hi) / radius; JACOBI (L != null): L L^T = bsum + D2 (- sub, in bsum's layout, when given) per column
// block, flags[kCgFail] where that fails
void launch_cgnr_precond_factor(const CgnrCols& C, const double* bsum, double lo, double hi, double radius, double* D2, double* L, int* flags, hipStream_t s,
                                const double* sub = nullptr);

// w = J v.  v = fma(beta, p, z) with beta = scal[kCgBeta] (p != null), else v = z.  flags (may be null): the done flag.
void launch_cgnr_jp(const CgnrJac& J, const double* z, const double* p, const double* scal, double* w, const int* flags, hipStream_t s);
// q = J^T w (+ D2 v).  kCgnrJtwCg: v = p <- fma(beta, p, z), written by the launch that owns the block; kCgnrJtwVector: v = z as
// it is; kCgnrJtwPlain: no vector, no D2.  partial: [num_partials * kCgnrLanes]
// kCgnrJtwNegated: q = -J^T w.
enum { kCgnrJtwCg = 0, kCgnrJtwVector = 1, kCgnrJtwPlain = 2, kCgnrJtwNegated = 3 };
void launch_cgnr_jtw(int mode, const CgnrJac& J, const CgnrCols& C, const double* w, const double* D2, const double* z, double* p, const double* scal,
                     double* q, double* partial, const int* flags, hipStream_t s);
// partials[chunk] = sum a_i b_i (kind 0) or sum a_i (b_i + a_i / 2) (kind 1) over chunks of kCgnrDotChunk
void launch_cgnr_dot(int kind, const double* a, const double* b, int n, double* partials, const int* flags, hipStream_t s);
// *out = sum of n partials (one workgroup)
void launch_cgnr_sum(const double* partials, int n, double* out, const int* flags, hipStream_t s);
// x += alpha p (before the products of a residual reset)
void launch_cgnr_axpy(const double* scal, const double* p, double* x, int n, const int* flags, hipStream_t s);
// The fused update, one lane per column block: kCgnrInit res = b (x = 0); kCgnrStep x += alpha p, res -= alpha q; kCgnrReset
// res = b - q (q = A x).  Then z = M^-1 res (L == null: z = res) and per workgroup the partials of res . z, x . (b + res), b . b
// at partials[3 * workgroup + 0..2].
enum { kCgnrInit = 0, kCgnrStep = 1, kCgnrReset = 2 };
void launch_cgnr_update(int mode, const CgnrCols& C, const double* L, const double* b, const double* p, const double* q, const double* scal,
                        double* x, double* res, double* z, double* partials, const int* flags, hipStream_t s);
// The three scalar kernels (one workgroup each; nparts: first-stage workgroups of the launch before)
void launch_cgnr_scalar_init(const double* partials3, int nparts, double* scal, int* flags, hipStream_t s);
void launch_cgnr_scalar_alpha(const double* partials, int nparts, double* scal, int* flags, hipStream_t s);
void launch_cgnr_scalar_end(const double* partials3, int nparts, double eta, int min_it, int max_it, double* scal, int* flags, hipStream_t s);

// --- the Schur elimination (cgnr_plan.hpp) -----------------------------------------------------------------------------------------
// E: the e-blocks as column blocks with their slot lists and parts; long_slots[2 l], [2 l + 1]: the range of E.cb_slots of long
// e-block l.  L: the factors of V_e = bsum_e + D2_e in E.cb_moff's places.  t_e = J_e^T w in plan order, then
//   kCgnrElimProject: w <- w - J_e V_e^-1 t_e on the rows of e (no two e-blocks share a row);
//   kCgnrElimBacksub: y_e = V_e^-1 (b_e - t_e), w untouched.
// partial: [E's num_partials * kCgnrLanes]
enum { kCgnrElimProject = 0, kCgnrElimBacksub = 1 };
void launch_cgnr_eliminate(int mode, const CgnrJac& J, const CgnrCols& E, const int* long_slots, const double* L, const double* b, double* w, double* y,
                           double* partial, const int* flags, hipStream_t s);
// The pairs (F block g, e-neighbour) of the block diagonal of S and the parts of the pair lists.
struct CgnrPairs {
  int num_parts, num_long;
  const int* part_f; const int* part_begin; const int* part_end; const int* part_out;
  const int* long_f; const int* long_begin;
  const int* pair_e;           // per pair: the e-block as a column block of the full list ...
  const int* cb_size; const int* cb_moff;  // ... whose sizes and matrix offsets these are
  const int* pair_slot_begin; const int* slot_g; const int* slot_e;
};
// sdiag[F.cb_moff[g] + a * size + b] = sum over the pairs (g, e) of (L_e^-1 W_ge^T)^T (L_e^-1 W_ge^T), W_ge summed over the
// pair's terms first; partial: [P's num_partials * 256]
void launch_cgnr_schur_diag(const CgnrJac& J, const CgnrCols& F, const CgnrPairs& P, const double* L, double* sdiag, double* partial, hipStream_t s);

// --- the candidate -----------------------------------------------------------------------------------------------------------------
// x_new = x (+) (y scale) per parameter block; partials[workgroup] of |x - x_new|^2
void launch_cgnr_candidate(const ParamBlock* pblocks, int num_pb, const double* y, const double* scale, const double* x, double* x_new, double* partials, hipStream_t s);

}  // namespace sk
