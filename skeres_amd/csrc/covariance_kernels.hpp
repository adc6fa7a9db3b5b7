// Launchers of covariance_kernels.hip: the normal matrix of a block-sparse Jacobian, its scaling, the border of selected columns,
// the pivot ratio of the factor and the extraction of the requested covariance blocks (plan: covariance_plan.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"

namespace sk {

// the Jacobian as Problem::Evaluate leaves it on the device
struct CovJac {
  const double* values;
  const int* val_off;     // [residual blocks + 1]
  const int* row_off;     // [residual blocks + 1]
  const int* slot_owner;  // per slot: its residual block
  const int* slot_pos;    // per slot: first value inside a row of its residual block
};

struct CovPairs {
  int num_parts, num_long;
  const int* part_pair; const int* part_begin; const int* part_end; const int* part_out;
  const int* long_pair; const int* long_begin;
  const int* pair_i; const int* pair_j;  // column blocks
  const int* term_si; const int* term_sj;
  const int* cb_col; const int* cb_size;
};

struct CovRequests {
  int num;
  const int* ra; const int* rb;            // first row / column in the k x k result (-1: zero block, nothing is written)
  const int* a; const int* b;              // parameter blocks
  const long* tan_off; const long* amb_off;
  const ParamBlock* pblocks;               // per parameter block (local_off: first column of H, -1: none)
  const double* x;                         // every parameter block of the problem, one after the other
};

// H (lower triangle, row-major, ld) += sum J_i^T J_j per pair; H zeroed by the caller.  partial: num_partials x kCovarianceTile.
void launch_cov_normal_assemble(const CovJac& J, const CovPairs& P, double* H, long ld, double* partial, hipStream_t s);
// d = diag(H)^(-1/2) over the n columns (1 on the padding up to npad_h, whose diagonal becomes 1); *zero_col = the first column whose
// diagonal entry is exactly 0 (unchanged when there is none: the caller sets it to INT_MAX); then H <- D H D on the lower triangle and
// the unit rows e_{sel_col[t]} in rows npad_h + t.
void launch_cov_scale(double* H, long ld, int n, int npad_h, double* d, int* zero_col, const int* sel_col, int k, hipStream_t s);
// out[0] = min, out[1] = max of L_jj^2 over the n columns, in a fixed order
void launch_cov_pivot_ratio(const double* L, long ld, int n, double* out, hipStream_t s);
// border: the k x k block behind the factored columns (lower triangle), holding -Sel^T (D H D)^-1 Sel
void launch_cov_extract(const CovRequests& R, const double* border, long ld, const double* d, double* out, hipStream_t s);

}  // namespace sk
