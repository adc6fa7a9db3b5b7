// HIP kernels of sk_covariance_compute (gfx950, wave64, fp64): the normal matrix H = J^T J of the block-sparse Jacobian that
// Problem::Evaluate leaves on the device, its diagonal scaling with the border of selected unit rows, the pivot ratio of the factor
// and the extraction (and lift) of the requested blocks.  They stream HBM; every sum runs in an order that the plan fixes
// (covariance_plan.hpp), without floating-point atomics.  The factorisation between them is cholesky_factor (chol_kernels.hip).
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
    else if (ci != cj || a >= b) H[(row0 + a) * ld + col0 + b] = s;
  }
}
__global__ __launch_bounds__(64) void cov_normal_assemble_long_kernel(CovPairs P, double* __restrict__ H, long ld, const double* __restrict__ partial) {
  const int q = P.long_pair[blockIdx.x], ci = P.pair_i[q], cj = P.pair_j[q];
  const int ni = P.cb_size[ci], nj = P.cb_size[cj], begin = P.long_begin[blockIdx.x], end = P.long_begin[blockIdx.x + 1];
  const long row0 = P.cb_col[ci], col0 = P.cb_col[cj];
  for (int e = threadIdx.x; e < ni * nj; e += 64) {
    const int a = e / nj, b = e - a * nj;
    double s = 0.0;
    for (int k = begin; k < end; ++k) s += partial[(size_t)k * kCovarianceTile + e];
    if (ci != cj || a >= b) H[(row0 + a) * ld + col0 + b] = s;
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
}  // namespace
__global__ __launch_bounds__(256) void cov_extract_kernel(CovRequests R, const double* __restrict__ border, long ld, const double* __restrict__ d, double* __restrict__ out) {
  __shared__ double T[kCovarianceTile], M[kCovarianceTile], Pa[kCovarianceTile], Pb[kCovarianceTile];
  const int r = blockIdx.x, ra = R.ra[r], rb = R.rb[r];
  if (ra < 0 || rb < 0) return;  // (a constant block: the output's zeros stand; the whole workgroup leaves)
  const ParamBlock pa = R.pblocks[R.a[r]], pb = R.pblocks[R.b[r]];
  const int ta = pa.local_size, tb = pb.local_size, ga = pa.global_size, gb = pb.global_size;
  const int e = threadIdx.x;
  if (e < ta * tb) {
    const int a = e / tb, b = e - a * tb;
    const int row = ra + a, col = rb + b;
    const double v = row >= col ? border[(long)row * ld + col] : border[(long)col * ld + row];
    const double t = -v * (d[pa.local_off + a] * d[pb.local_off + b]);
    T[e] = t;
    out[R.tan_off[r] + e] = t;
  }
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
void launch_cov_extract(const CovRequests& R, const double* border, long ld, const double* d, double* out, hipStream_t s) {
  if (R.num > 0) hipLaunchKernelGGL(cov_extract_kernel, dim3(R.num), dim3(256), 0, s, R, border, ld, d, out);
}

}  // namespace sk
