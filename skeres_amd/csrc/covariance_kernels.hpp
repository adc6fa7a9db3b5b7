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
  const int* cb_col; const int* cb_size;  // cb_col: the block's first column of the matrix the pairs are summed into
  // Schur elimination (nullptr without it): per pair its tile of `tiles` (-1: the dense matrix) and whether the tile is stored transposed
  const int* pair_tile = nullptr; const int* pair_flip = nullptr; double* tiles = nullptr;
};

struct CovRequests {
  int num;
  const int* ra; const int* rb;            // first row / column in the k x k result (-1: zero block, nothing is written)
  const int* a; const int* b;              // parameter blocks
  const long* tan_off; const long* amb_off;
  const ParamBlock* pblocks;               // per parameter block (local_off: first column of H, -1: none)
  const double* x;                         // every parameter block of the problem, one after the other
};

// Schur elimination (covariance_plan.hpp): the e-blocks, F(e), the tiles and the Schur terms as the plan lists them
struct CovSchur {
  int num_cb, num_e;
  const int* cb_col; const int* cb_red; const int* cb_size; const int* cb_elim;  // per column block: first column of H; cb_red as in the plan
  const int* e_cb;                                                             // [num_e]
  const int* ew_begin; const int* ew_tile; const int* ew_g; const int* ew_sel;   // F(e)
  double* tiles;                                                               // tile t < num_e: V_e, then L_e; num_e + t: L_e^-1; then (g, e): W_ge, then X_ge
  int num_parts, num_long;
  const int* part_pair; const int* part_begin; const int* part_end; const int* part_out;
  const int* long_pair; const int* long_begin; const int* pair_i; const int* pair_j;
  const int* term_a; const int* term_b; const int* term_ne;
  const int* req_ea; const int* req_eb;                                        // per request: e-block index of a / b (-1: in F)
};

// d[column of H] = diag(H)^(-1/2) over ALL columns: from the V tiles (e-blocks) and from the dense U (F blocks); *zero_col as launch_cov_scale
void launch_cov_schur_diag(const CovSchur& Sc, const double* U, long ld, double* d, int* zero_col, hipStream_t s);
// per e-block: V~_e = D_e V_e D_e = L_e L_e^T (tile e <- L_e, tile num_e + e <- L_e^-1), slot[2 e], slot[2 e + 1] = min, max of L_jj^2,
// *info = 1 on a pivot that is not positive, every (g, e) tile <- X_ge = D_g W_ge D_e L_e^-T
void launch_cov_schur_eblocks(const CovSchur& Sc, const double* d, double* slot, int* info, hipStream_t s);
// S~_gg' -= sum_e X_ge X_g'e^T on the lower triangle of the scaled U, terms in plan order; partial: num_spartials x kCovarianceTile
void launch_cov_schur_update(const CovSchur& Sc, double* S, long ld, double* partial, hipStream_t s);
// out[0] = min(out[0], slots' minima), out[1] = max(out[1], slots' maxima), in a fixed order (out: launch_cov_pivot_ratio's of S~'s factor)
void launch_cov_schur_pivot_ratio(const double* slot, int num_e, double* out, hipStream_t s);
// launch_cov_extract with the back-substitution of the eliminated blocks (R.ra / R.rb: rows of an F block; Sc.req_ea / req_eb >= 0: an e-block)
void launch_cov_schur_extract(const CovRequests& R, const CovSchur& Sc, const double* border, long ld, const double* d, double* out, hipStream_t s);

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
