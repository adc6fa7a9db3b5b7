// HIP kernels of sk_covariance_compute (gfx950, wave64, fp64): the normal matrix H = J^T J of the block-sparse Jacobian that
// Problem::Evaluate leaves on the device, its diagonal scaling with the border of selected unit rows, the pivot ratio of the factor
// and the extraction (and lift) of the requested blocks.  They stream HBM; every sum runs in an order that the plan fixes
// (covariance_plan.hpp), without floating-point atomics.  The factorisation between them is cholesky_factor (chol_kernels.hip).
// The kernels of the Schur elimination (the e-blocks' factors, the Schur update, the back-substituting extraction) are at the end.
#include <hip/hip_runtime.h>

#include "covariance_kernels.hpp"
#include "covariance_plan.hpp"

namespace sk {

// ---- H += J_i^T J_j ------------------------------------------------------------------------------------------------------------------
// One wave per part: lane e (e, e + 64, ... below size_i x size_j) owns entry (a, b) of the pair's tile and walks the part's terms in
// plan order, so consecutive lanes store along a row of H.  The only part of a pair stores into H (a diagonal pair: its lower
// triangle); the parts of a long pair leave partial tiles that cov_normal_assemble_long_kernel adds entry by entry, in part order.
__global__ __launch_bounds__(64) void cov_normal_assemble_kernel(CovJac J, CovPairs P, double* __restrict__ H, long ld, double* __restrict__ partial) {
  const int part = blockIdx.x;
  const int q = P.part_pair[part], ci = P.pair_i[q], cj = P.pair_j[q];
  const int ni = P.cb_size[ci], nj = P.cb_size[cj], begin = P.part_begin[part], end = P.part_end[part], out = P.part_out[part];
  const int tile = P.pair_tile ? P.pair_tile[q] : -1;  // (Schur elimination: a pair that involves an e-block sums into its tile)
  const long row0 = P.cb_col[ci], col0 = P.cb_col[cj];
  for (int e = threadIdx.x; e < ni * nj; e += 64) {
    const int a = e / nj, b = e - a * nj;
    double s = 0.0;
    for (int k = begin; k < end; ++k) {
      const int si = P.term_si[k], sj = P.term_sj[k], i = J.slot_owner[si];
      const int nres = J.row_off[i + 1] - J.row_off[i];
      const int width = (J.val_off[i + 1] - J.val_off[i]) / nres;
      const double* vi = J.values + J.val_off[i] + J.slot_pos[si] + a;
      const double* vj = J.values + J.val_off[i] + J.slot_pos[sj] + b;
      for (int r = 0; r < nres; ++r) s += vi[(size_t)r * width] * vj[(size_t)r * width];
    }
    if (out >= 0) partial[(size_t)out * kCovarianceTile + e] = s;
    else if (tile >= 0) P.tiles[(size_t)tile * kCovarianceTile + (P.pair_flip[q] ? b * ni + a : e)] = s;
    else if (ci != cj || a >= b) H[(row0 + a) * ld + col0 + b] = s;
  }
}
__global__ __launch_bounds__(64) void cov_normal_assemble_long_kernel(CovPairs P, double* __restrict__ H, long ld, const double* __restrict__ partial) {
  const int q = P.long_pair[blockIdx.x], ci = P.pair_i[q], cj = P.pair_j[q];
  const int ni = P.cb_size[ci], nj = P.cb_size[cj], begin = P.long_begin[blockIdx.x], end = P.long_begin[blockIdx.x + 1];
  const int tile = P.pair_tile ? P.pair_tile[q] : -1;
  const long row0 = P.cb_col[ci], col0 = P.cb_col[cj];
  for (int e = threadIdx.x; e < ni * nj; e += 64) {
    const int a = e / nj, b = e - a * nj;
    double s = 0.0;
    for (int k = begin; k < end; ++k) s += partial[(size_t)k * kCovarianceTile + e];
    if (tile >= 0) P.tiles[(size_t)tile * kCovarianceTile + (P.pair_flip[q] ? b * ni + a : e)] = s;
    else if (ci != cj || a >= b) H[(row0 + a) * ld + col0 + b] = s;
  }
}
void launch_cov_normal_assemble(const CovJac& J, const CovPairs& P, double* H, long ld, double* partial, hipStream_t s) {
  if (P.num_parts > 0) hipLaunchKernelGGL(cov_normal_assemble_kernel, dim3(P.num_parts), dim3(64), 0, s, J, P, H, ld, partial);
  if (P.num_long > 0) hipLaunchKernelGGL(cov_normal_assemble_long_kernel, dim3(P.num_long), dim3(64), 0, s, P, H, ld, (const double*)partial);
}

// ---- H <- D H D, the border ------------------------------------------------------------------------------------------------------------
// d first (a launch of its own: every entry of H below reads two of them), with the padding's unit diagonal and the border's unit
// rows; an exact zero on the diagonal is flagged with its column (an integer minimum: the first one, whatever the order of arrival).
__global__ __launch_bounds__(256) void cov_scale_diag_kernel(double* __restrict__ H, long ld, int n, int npad_h, double* __restrict__ d, int* zero_col,
                                                             const int* __restrict__ sel_col, int k) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < n) {
    const double h = H[(long)j * ld + j];
    if (h == 0.0) atomicMin(zero_col, j);
    d[j] = 1.0 / sqrt(h);
  } else if (j < npad_h) {
    d[j] = 1.0;
    H[(long)j * ld + j] = 1.0;
  }
  if (j < k) H[(long)(npad_h + j) * ld + sel_col[j]] = 1.0;
}
// blockIdx.y: the row; the row's entries up to the diagonal
__global__ __launch_bounds__(256) void cov_scale_kernel(double* __restrict__ H, long ld, int n, const double* __restrict__ d) {
  const int i = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (i >= n || j > i) return;
  H[(long)i * ld + j] *= d[i] * d[j];
}
void launch_cov_scale(double* H, long ld, int n, int npad_h, double* d, int* zero_col, const int* sel_col, int k, hipStream_t s) {
  const int m = npad_h > k ? npad_h : k;
  if (m > 0) hipLaunchKernelGGL(cov_scale_diag_kernel, dim3((m + 255) / 256), dim3(256), 0, s, H, ld, n, npad_h, d, zero_col, sel_col, k);
  if (n > 0) hipLaunchKernelGGL(cov_scale_kernel, dim3((n + 255) / 256, n), dim3(256), 0, s, H, ld, n, (const double*)d);
}

// ---- min and max of L_jj^2 ---------------------------------------------------------------------------------------------------------------
// One workgroup: thread t takes the columns t, t + 256, ... in order, then a fixed tree over the 256 threads.
__global__ __launch_bounds__(256) void cov_pivot_ratio_kernel(const double* __restrict__ L, long ld, int n, double* out) {
  __shared__ double lo[256], hi[256];
  double mn = INFINITY, mx = 0.0;
  for (int j = threadIdx.x; j < n; j += 256) {
    const double v = L[(long)j * ld + j], sq = v * v;
    mn = fmin(mn, sq); mx = fmax(mx, sq);
  }
  lo[threadIdx.x] = mn; hi[threadIdx.x] = mx;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) { lo[threadIdx.x] = fmin(lo[threadIdx.x], lo[threadIdx.x + w]); hi[threadIdx.x] = fmax(hi[threadIdx.x], hi[threadIdx.x + w]); }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out[0] = lo[0]; out[1] = hi[0]; }
}
void launch_cov_pivot_ratio(const double* L, long ld, int n, double* out, hipStream_t s) {
  hipLaunchKernelGGL(cov_pivot_ratio_kernel, dim3(1), dim3(256), 0, s, L, ld, n, out);
}

// ---- the requested blocks ----------------------------------------------------------------------------------------------------------------
// One workgroup per requested pair (a, b).  Tangent: T = d_a d_b (H~^-1)_ab, the border block negated (its lower triangle is read:
// entry (r, c) with r < c comes from (c, r)).  Ambient: P_a T P_b^T with P = dPlus/ddelta at x — identity and subset blocks copy
// (scatter) their rows / columns, the other parameterizations go through param_jacobian.
namespace {
// row of the tangent block that ambient coordinate i of a copying parameterization takes (-1: held, a zero row); -2: P is dense
__device__ inline int cov_copy_index(const ParamBlock& p, int i) {
  if (p.type == kParamIdentity) return i;
  if (p.type == kParamSubset) return ((p.constant_mask >> i) & 1u) ? -1 : __popc(~p.constant_mask & ((1u << i) - 1u));
  return -2;
}
// the ambient block of request r from its tangent block T (filled by the calling workgroup of 256; no barrier behind it yet)
__device__ __forceinline__ void cov_lift(const CovRequests& R, int r, const ParamBlock& pa, const ParamBlock& pb, const double* T, double* M, double* Pa, double* Pb,
                                         double* __restrict__ out) {
  const int ta = pa.local_size, tb = pb.local_size, ga = pa.global_size, gb = pb.global_size;
  const int e = threadIdx.x;
  if (e == 0 && cov_copy_index(pa, 0) == -2) param_jacobian(pa, R.x + pa.global_off, Pa);
  if (e == 64 && cov_copy_index(pb, 0) == -2) param_jacobian(pb, R.x + pb.global_off, Pb);
  __syncthreads();
  if (e < ga * tb) {  // M = P_a T
    const int i = e / tb, b = e - i * tb;
    const int src = cov_copy_index(pa, i);
    double s = 0.0;
    if (src >= 0) s = T[src * tb + b];
    else if (src == -2) for (int a = 0; a < ta; ++a) s += Pa[i * ta + a] * T[a * tb + b];
    M[e] = s;
  }
  __syncthreads();
  if (e < ga * gb) {  // M P_b^T; a diagonal block (a == b) takes entry (i, j), i < j, as (j, i) is computed: symmetric bit for bit
    int i = e / gb, j = e - i * gb;
    if (R.a[r] == R.b[r] && i < j) { const int t = i; i = j; j = t; }
    const int src = cov_copy_index(pb, j);
    double s = 0.0;
    if (src >= 0) s = M[i * tb + src];
    else if (src == -2) for (int b = 0; b < tb; ++b) s += M[i * tb + b] * Pb[j * tb + b];
    out[R.amb_off[r] + e] = s;
  }
}
}  // namespace
__global__ __launch_bounds__(256) void cov_extract_kernel(CovRequests R, const double* __restrict__ border, long ld, const double* __restrict__ d, double* __restrict__ out) {
  __shared__ double T[kCovarianceTile], M[kCovarianceTile], Pa[kCovarianceTile], Pb[kCovarianceTile];
  const int r = blockIdx.x, ra = R.ra[r], rb = R.rb[r];
  if (ra < 0 || rb < 0) return;  // (a constant block: the output's zeros stand; the whole workgroup leaves)
  const ParamBlock pa = R.pblocks[R.a[r]], pb = R.pblocks[R.b[r]];
  const int ta = pa.local_size, tb = pb.local_size;
  const int e = threadIdx.x;
  if (e < ta * tb) {
    const int a = e / tb, b = e - a * tb;
    const int row = ra + a, col = rb + b;
    const double v = row >= col ? border[(long)row * ld + col] : border[(long)col * ld + row];
    const double t = -v * (d[pa.local_off + a] * d[pb.local_off + b]);
    T[e] = t;
    out[R.tan_off[r] + e] = t;
  }
  cov_lift(R, r, pa, pb, T, M, Pa, Pb, out);
}
void launch_cov_extract(const CovRequests& R, const double* border, long ld, const double* d, double* out, hipStream_t s) {
  if (R.num > 0) hipLaunchKernelGGL(cov_extract_kernel, dim3(R.num), dim3(256), 0, s, R, border, ld, d, out);
}

// ---- Schur elimination -------------------------------------------------------------------------------------------------------------------
// H = [[U, W], [W^T, V]], V block diagonal over the e-blocks (covariance_plan.hpp).  d over all columns; per e-block the factor of
// V~_e and X_ge = D_g W_ge D_e L_e^-T in place of W_ge; S~ = D U D - sum_e X_ge X_g'e^T, which cholesky_factor takes with the border;
// the extraction substitutes back.  A tile is kCovarianceTile doubles, row-major with the e-block's tangent size as its row length.
// One thread per column block.
__global__ __launch_bounds__(256) void cov_schur_diag_kernel(CovSchur Sc, const double* __restrict__ U, long ld, double* __restrict__ d, int* zero_col) {
  const int cb = blockIdx.x * 256 + threadIdx.x;
  if (cb >= Sc.num_cb) return;
  const int n = Sc.cb_size[cb], col = Sc.cb_col[cb], red = Sc.cb_red[cb];
  for (int a = 0; a < n; ++a) {
    const double h = Sc.cb_elim[cb] ? Sc.tiles[(size_t)red * kCovarianceTile + a * n + a] : U[(long)(red + a) * ld + red + a];
    if (h == 0.0) atomicMin(zero_col, col + a);
    d[col + a] = 1.0 / sqrt(h);
  }
}
void launch_cov_schur_diag(const CovSchur& Sc, const double* U, long ld, double* d, int* zero_col, hipStream_t s) {
  if (Sc.num_cb > 0) hipLaunchKernelGGL(cov_schur_diag_kernel, dim3((Sc.num_cb + 255) / 256), dim3(256), 0, s, Sc, U, ld, d, zero_col);
}

// One wave per e-block: lane 0 factors the block of at most 16 columns and inverts its factor (a serial chain either way), then the
// wave walks F(e), one tile after the other through LDS.
__global__ __launch_bounds__(64) void cov_schur_eblock_kernel(CovSchur Sc, const double* __restrict__ d, double* __restrict__ slot, int* info) {
  __shared__ double L[kCovarianceTile], Li[kCovarianceTile], W[kCovarianceTile];
  const int e = blockIdx.x, cb = Sc.e_cb[e], ne = Sc.cb_size[cb], t = threadIdx.x;
  const double* de = d + Sc.cb_col[cb];
  double* V = Sc.tiles + (size_t)e * kCovarianceTile;
  double* Vi = Sc.tiles + (size_t)(Sc.num_e + e) * kCovarianceTile;
  for (int i = t; i < ne * ne; i += 64) {
    const int a = i / ne, b = i - a * ne;
    L[i] = a >= b ? V[i] * (de[a] * de[b]) : 0.0;
    Li[i] = 0.0;
  }
  __syncthreads();
  if (t == 0) {
    double mn = INFINITY, mx = 0.0;
    bool bad = false;
    for (int j = 0; j < ne; ++j) {
      double dj = L[j * ne + j];
      for (int k = 0; k < j; ++k) dj -= L[j * ne + k] * L[j * ne + k];
      if (!(dj > 0.0) || !isfinite(dj)) bad = true;
      mn = fmin(mn, dj); mx = fmax(mx, dj);
      const double l = sqrt(dj);
      L[j * ne + j] = l;
      for (int i = j + 1; i < ne; ++i) {
        double s = L[i * ne + j];
        for (int k = 0; k < j; ++k) s -= L[i * ne + k] * L[j * ne + k];
        L[i * ne + j] = s / l;
      }
    }
    for (int i = 0; i < ne; ++i)
      for (int j = 0; j <= i; ++j) {
        double s = i == j ? 1.0 : 0.0;
        for (int k = j; k < i; ++k) s -= L[i * ne + k] * Li[k * ne + j];
        Li[i * ne + j] = s / L[i * ne + i];
      }
    slot[2 * e] = bad ? 0.0 : mn; slot[2 * e + 1] = mx;
    if (bad) atomicMax(info, 1);
  }
  __syncthreads();
  for (int i = t; i < ne * ne; i += 64) { V[i] = L[i]; Vi[i] = Li[i]; }
  for (int k = Sc.ew_begin[e]; k < Sc.ew_begin[e + 1]; ++k) {
    double* Wt = Sc.tiles + (size_t)Sc.ew_tile[k] * kCovarianceTile;
    const int g = Sc.ew_g[k], ng = Sc.cb_size[g];
    const double* dg = d + Sc.cb_col[g];
    for (int i = t; i < ng * ne; i += 64) {
      const int a = i / ne, b = i - a * ne;
      W[i] = Wt[i] * (dg[a] * de[b]);
    }
    __syncthreads();
    for (int i = t; i < ng * ne; i += 64) {  // X = W~ L^-T: entry (a, c) takes row c of L^-1
      const int a = i / ne, c = i - a * ne;
      double s = 0.0;
      for (int b = 0; b <= c; ++b) s += W[a * ne + b] * Li[c * ne + b];
      Wt[i] = s;
    }
    __syncthreads();
  }
}
void launch_cov_schur_eblocks(const CovSchur& Sc, const double* d, double* slot, int* info, hipStream_t s) {
  if (Sc.num_e > 0) hipLaunchKernelGGL(cov_schur_eblock_kernel, dim3(Sc.num_e), dim3(64), 0, s, Sc, d, slot, info);
}

// One wave per part of a pair's Schur terms, one lane per entry of the pair's block (as cov_normal_assemble_kernel); the only part
// of a pair subtracts from S~ (a diagonal pair: from its lower triangle), the parts of a long pair leave partial tiles.
__global__ __launch_bounds__(64) void cov_schur_update_kernel(CovSchur Sc, double* __restrict__ S, long ld, double* __restrict__ partial) {
  const int part = blockIdx.x;
  const int q = Sc.part_pair[part], ci = Sc.pair_i[q], cj = Sc.pair_j[q];
  const int ni = Sc.cb_size[ci], nj = Sc.cb_size[cj], begin = Sc.part_begin[part], end = Sc.part_end[part], out = Sc.part_out[part];
  const long row0 = Sc.cb_red[ci], col0 = Sc.cb_red[cj];
  for (int e = threadIdx.x; e < ni * nj; e += 64) {
    const int a = e / nj, b = e - a * nj;
    double s = 0.0;
    for (int k = begin; k < end; ++k) {
      const int ne = Sc.term_ne[k];
      const double* xa = Sc.tiles + (size_t)Sc.term_a[k] * kCovarianceTile + a * ne;
      const double* xb = Sc.tiles + (size_t)Sc.term_b[k] * kCovarianceTile + b * ne;
      for (int c = 0; c < ne; ++c) s += xa[c] * xb[c];
    }
    if (out >= 0) partial[(size_t)out * kCovarianceTile + e] = s;
    else if (ci != cj || a >= b) S[(row0 + a) * ld + col0 + b] -= s;
  }
}
__global__ __launch_bounds__(64) void cov_schur_update_long_kernel(CovSchur Sc, double* __restrict__ S, long ld, const double* __restrict__ partial) {
  const int q = Sc.long_pair[blockIdx.x], ci = Sc.pair_i[q], cj = Sc.pair_j[q];
  const int ni = Sc.cb_size[ci], nj = Sc.cb_size[cj], begin = Sc.long_begin[blockIdx.x], end = Sc.long_begin[blockIdx.x + 1];
  const long row0 = Sc.cb_red[ci], col0 = Sc.cb_red[cj];
  for (int e = threadIdx.x; e < ni * nj; e += 64) {
    const int a = e / nj, b = e - a * nj;
    double s = 0.0;
    for (int k = begin; k < end; ++k) s += partial[(size_t)k * kCovarianceTile + e];
    if (ci != cj || a >= b) S[(row0 + a) * ld + col0 + b] -= s;
  }
}
void launch_cov_schur_update(const CovSchur& Sc, double* S, long ld, double* partial, hipStream_t s) {
  if (Sc.num_parts > 0) hipLaunchKernelGGL(cov_schur_update_kernel, dim3(Sc.num_parts), dim3(64), 0, s, Sc, S, ld, partial);
  if (Sc.num_long > 0) hipLaunchKernelGGL(cov_schur_update_long_kernel, dim3(Sc.num_long), dim3(64), 0, s, Sc, S, ld, (const double*)partial);
}

// The pivots of every L_e beside those of S~'s factor: together the pivots of the factor of H~ with E ordered first.
__global__ __launch_bounds__(256) void cov_schur_pivot_ratio_kernel(const double* __restrict__ slot, int num_e, double* out) {
  __shared__ double lo[256], hi[256];
  double mn = INFINITY, mx = 0.0;
  for (int e = threadIdx.x; e < num_e; e += 256) { mn = fmin(mn, slot[2 * e]); mx = fmax(mx, slot[2 * e + 1]); }
  lo[threadIdx.x] = mn; hi[threadIdx.x] = mx;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) { lo[threadIdx.x] = fmin(lo[threadIdx.x], lo[threadIdx.x + w]); hi[threadIdx.x] = fmax(hi[threadIdx.x], hi[threadIdx.x + w]); }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out[0] = fmin(out[0], lo[0]); out[1] = fmax(out[1], hi[0]); }
}
void launch_cov_schur_pivot_ratio(const double* slot, int num_e, double* out, hipStream_t s) {
  hipLaunchKernelGGL(cov_schur_pivot_ratio_kernel, dim3(1), dim3(256), 0, s, slot, num_e, out);
}

// One workgroup per requested pair.  C~ = H~^-1 over F is the border, negated; with X and L^-1 of the e-blocks
//   (f, e)   C~_fe  = -(sum_{g in F(e)} C~_fg X_ge) L_e^-1
//   (e, e')  C~_ee' = L_e^-T (delta_ee' I + sum_{g in F(e)} sum_{g' in F(e')} X_ge^T C~_gg' X_g'e') L_e'^-1
// The double sum runs per row a of the block: thread t takes g' = t, t + 256, ... of F(e'), walks F(e) in plan order for each, and the
// 256 partial rows are added through a fixed tree in LDS.  Then d_a d_b and the lift, as cov_extract_kernel.
__global__ __launch_bounds__(256) void cov_schur_extract_kernel(CovRequests R, CovSchur Sc, const double* __restrict__ border, long ld, const double* __restrict__ d,
                                                                double* __restrict__ out) {
  __shared__ double T[kCovarianceTile], M[kCovarianceTile], Pa[kCovarianceTile], Pb[kCovarianceTile], Y[kCovarianceTile], red[256];
  const int r = blockIdx.x, ra = R.ra[r], rb = R.rb[r];
  if (ra < 0 || rb < 0) return;  // (a constant block: the output's zeros stand; the whole workgroup leaves)
  const ParamBlock pa = R.pblocks[R.a[r]], pb = R.pblocks[R.b[r]];
  const int ta = pa.local_size, tb = pb.local_size, ea = Sc.req_ea[r], eb = Sc.req_eb[r];
  const int t = threadIdx.x;
  auto Ct = [&](int row, int col) { return -(row >= col ? border[(long)row * ld + col] : border[(long)col * ld + row]); };
  if (ea < 0 && eb < 0) {
    if (t < ta * tb) { const int a = t / tb, b = t - a * tb; T[t] = Ct(ra + a, rb + b); }
  } else if (ea < 0 || eb < 0) {
    const bool a_is_f = ea < 0;
    const int e = a_is_f ? eb : ea, rf = a_is_f ? ra : rb, tf = a_is_f ? ta : tb, te = a_is_f ? tb : ta;
    const double* Li = Sc.tiles + (size_t)(Sc.num_e + e) * kCovarianceTile;
    if (t < tf * te) {
      const int f = t / te, c = t - f * te;
      double s = 0.0;
      for (int k = Sc.ew_begin[e]; k < Sc.ew_begin[e + 1]; ++k) {
        const double* X = Sc.tiles + (size_t)Sc.ew_tile[k] * kCovarianceTile;
        const int ng = Sc.cb_size[Sc.ew_g[k]], rg = Sc.ew_sel[k];
        for (int q = 0; q < ng; ++q) s += Ct(rf + f, rg + q) * X[q * te + c];
      }
      Y[t] = s;
    }
    __syncthreads();
    if (t < tf * te) {
      const int f = t / te, j = t - f * te;
      double s = 0.0;
      for (int c = j; c < te; ++c) s += Y[f * te + c] * Li[c * te + j];
      T[a_is_f ? f * te + j : j * tf + f] = -s;
    }
  } else {
    const double* La = Sc.tiles + (size_t)(Sc.num_e + ea) * kCovarianceTile;
    const double* Lb = Sc.tiles + (size_t)(Sc.num_e + eb) * kCovarianceTile;
    const int ka0 = Sc.ew_begin[ea], ka1 = Sc.ew_begin[ea + 1], kb0 = Sc.ew_begin[eb], kb1 = Sc.ew_begin[eb + 1];
    for (int a = 0; a < ta; ++a) {
      double acc[kCovarianceMaxBlock];
#pragma unroll
      for (int c = 0; c < kCovarianceMaxBlock; ++c) acc[c] = 0.0;
      for (int kb = kb0 + t; kb < kb1; kb += 256) {
        const double* Xb = Sc.tiles + (size_t)Sc.ew_tile[kb] * kCovarianceTile;
        const int ngb = Sc.cb_size[Sc.ew_g[kb]], rgb = Sc.ew_sel[kb];
        double w[kCovarianceMaxBlock];
#pragma unroll
        for (int q = 0; q < kCovarianceMaxBlock; ++q) w[q] = 0.0;
        for (int ka = ka0; ka < ka1; ++ka) {
          const double* Xa = Sc.tiles + (size_t)Sc.ew_tile[ka] * kCovarianceTile;
          const int nga = Sc.cb_size[Sc.ew_g[ka]], rga = Sc.ew_sel[ka];
          for (int p = 0; p < nga; ++p) {
            const double xa = Xa[p * ta + a];
#pragma unroll
            for (int q = 0; q < kCovarianceMaxBlock; ++q) if (q < ngb) w[q] += xa * Ct(rga + p, rgb + q);
          }
        }
#pragma unroll
        for (int q = 0; q < kCovarianceMaxBlock; ++q)
          if (q < ngb) {
#pragma unroll
            for (int c = 0; c < kCovarianceMaxBlock; ++c) if (c < tb) acc[c] += w[q] * Xb[q * tb + c];
          }
      }
#pragma unroll
      for (int c = 0; c < kCovarianceMaxBlock; ++c)
        if (c < tb) {  // (tb is the workgroup's: every thread meets the same barriers)
          red[t] = acc[c];
          __syncthreads();
          for (int w2 = 128; w2 > 0; w2 >>= 1) {
            if (t < w2) red[t] += red[t + w2];
            __syncthreads();
          }
          if (t == 0) M[a * tb + c] = red[0] + (ea == eb && a == c ? 1.0 : 0.0);
          __syncthreads();
        }
    }
    if (t < ta * tb) {  // Y = L_e^-T M
      const int i = t / tb, c = t - i * tb;
      double s = 0.0;
      for (int a = i; a < ta; ++a) s += La[a * ta + i] * M[a * tb + c];
      Y[t] = s;
    }
    __syncthreads();
    if (t < ta * tb) {  // Y L_e'^-1; a diagonal block keeps its lower triangle and mirrors it
      const int i = t / tb, j = t - i * tb;
      double s = 0.0;
      for (int c = j; c < tb; ++c) s += Y[i * tb + c] * Lb[c * tb + j];
      if (ea != eb) T[t] = s;
      else if (i >= j) { T[i * tb + j] = s; T[j * tb + i] = s; }
    }
  }
  __syncthreads();
  if (t < ta * tb) {
    const int a = t / tb, b = t - a * tb;
    const double v = T[t] * (d[pa.local_off + a] * d[pb.local_off + b]);
    T[t] = v;
    out[R.tan_off[r] + t] = v;
  }
  cov_lift(R, r, pa, pb, T, M, Pa, Pb, out);
}
void launch_cov_schur_extract(const CovRequests& R, const CovSchur& Sc, const double* border, long ld, const double* d, double* out, hipStream_t s) {
  if (R.num > 0) hipLaunchKernelGGL(cov_schur_extract_kernel, dim3(R.num), dim3(256), 0, s, R, Sc, border, ld, d, out);
}

}  // namespace sk
