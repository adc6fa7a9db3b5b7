// HIP kernels of the CGNR solver (gfx950, wave64, fp64): the two products with the block-sparse Jacobian, the block sums and the
// block-Jacobi preconditioner, the fused vector updates and the scalar kernels of the conjugate-gradient loop, and for the Schur
// elimination the projection w - J_E V^-1 J_E^T w and the block diagonal of the Schur complement.  All of them stream
// HBM; every sum runs in an order that the plan fixes (cgnr_plan.hpp), without floating-point atomics.  The kernels of the loop
// read the done flag first and return when it is set, so the host may enqueue iterations ahead of what the device will need.
#include <hip/hip_runtime.h>

#include "cgnr_kernels.hpp"
#include "cgnr_plan.hpp"

namespace sk {

namespace {

__device__ inline bool cg_done(const int* flags) { return flags && flags[kCgDone]; }
__device__ inline bool cg_bad(double v) { return !(v > 0.0) || !isfinite(v); }  // zero, negative or not finite

// sum over the workgroup's 256 threads in a fixed tree; the result in thread 0
__device__ inline double block_sum_256(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) { if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w]; __syncthreads(); }
  const double out = sh[0];
  __syncthreads();
  return out;
}
__device__ inline double block_max_256(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) { if ((int)threadIdx.x < w) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + w]); __syncthreads(); }
  const double out = sh[0];
  __syncthreads();
  return out;
}

}  // namespace

// ---- block sums -------------------------------------------------------------------------------------------------------------------
// One wave per part: lane e (e, e + 64, ... below size^2) owns entry (a, b) of the block's matrix and walks the part's slots in plan
// order.  A long block's parts are summed entry by entry, in part order, by the second launch.
__global__ __launch_bounds__(64) void cgnr_block_diag_kernel(CgnrJac J, CgnrCols C, double* bsum, double* partial, const int* flags) {
  if (cg_done(flags)) return;
  const int part = blockIdx.x;
  const int c = C.part_cb[part], size = C.cb_size[c], begin = C.part_begin[part], end = C.part_end[part], out = C.part_out[part];
  for (int e = threadIdx.x; e < size * size; e += 64) {
    const int a = e / size, b = e - a * size;
    double s = 0.0;
    for (int k = begin; k < end; ++k) {
      const int slot = C.cb_slots[k], i = J.slot_owner[slot];
      const int nres = J.row_off[i + 1] - J.row_off[i];
      const int width = (J.val_off[i + 1] - J.val_off[i]) / nres;
      const double* v = J.values + J.val_off[i] + J.slot_pos[slot];
      for (int r = 0; r < nres; ++r) s += v[(size_t)r * width + a] * v[(size_t)r * width + b];
    }
    if (out < 0) bsum[C.cb_moff[c] + e] = s; else partial[(size_t)out * 256 + e] = s;
  }
}
__global__ __launch_bounds__(64) void cgnr_block_diag_long_kernel(CgnrCols C, double* bsum, const double* partial, const int* flags) {
  if (cg_done(flags)) return;
  const int c = C.long_cb[blockIdx.x], size = C.cb_size[c];
  const int begin = C.long_begin[blockIdx.x], end = C.long_begin[blockIdx.x + 1];
  for (int e = threadIdx.x; e < size * size; e += 64) {
    double s = 0.0;
    for (int k = begin; k < end; ++k) s += partial[(size_t)k * 256 + e];
    bsum[C.cb_moff[c] + e] = s;
  }
}
void launch_cgnr_block_diag(const CgnrJac& J, const CgnrCols& C, double* bsum, double* partial, hipStream_t s, const int* flags) {
  if (C.num_parts > 0) hipLaunchKernelGGL(cgnr_block_diag_kernel, dim3(C.num_parts), dim3(64), 0, s, J, C, bsum, partial, flags);
  if (C.num_long > 0) hipLaunchKernelGGL(cgnr_block_diag_long_kernel, dim3(C.num_long), dim3(64), 0, s, C, bsum, (const double*)partial, flags);
}

// ---- Jacobi scaling ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cgnr_scale_compute_kernel(CgnrCols C, const double* bsum, double* scale) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C.num_cb) return;
  const int size = C.cb_size[c], col = C.cb_col[c];
  const double* m = bsum + C.cb_moff[c];
  for (int j = 0; j < size; ++j) scale[col + j] = 1.0 / (1.0 + sqrt(m[j * size + j]));
}
void launch_cgnr_scale_compute(const CgnrCols& C, const double* bsum, double* scale, hipStream_t s) {
  if (C.num_cb > 0) hipLaunchKernelGGL(cgnr_scale_compute_kernel, dim3((C.num_cb + 255) / 256), dim3(256), 0, s, C, bsum, scale);
}
// one lane per row, as cgnr_jp_kernel
__global__ __launch_bounds__(256) void cgnr_scale_apply_kernel(CgnrJac J, const double* scale) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= J.num_rows) return;
  const int i = J.row_block[row], r = row - J.row_off[i];
  const int nres = J.row_off[i + 1] - J.row_off[i];
  const int width = (J.val_off[i + 1] - J.val_off[i]) / nres;
  double* v = J.values + J.val_off[i] + (size_t)r * width;
  for (int slot = J.slot_begin[i]; slot < J.slot_begin[i + 1]; ++slot) {
    const int pos = J.slot_pos[slot];
    if (pos < 0) continue;
    const int col = J.slot_col[slot], size = J.slot_size[slot];
    for (int j = 0; j < size; ++j) v[pos + j] *= scale[col + j];
  }
}
void launch_cgnr_scale_apply(const CgnrJac& J, const double* scale, hipStream_t s) {
  if (J.num_rows > 0) hipLaunchKernelGGL(cgnr_scale_apply_kernel, dim3((J.num_rows + 255) / 256), dim3(256), 0, s, J, scale);
}

__global__ __launch_bounds__(256) void cgnr_gradient_norms_kernel(const double* gs, const double* scale, int n, const double* x, int ng, double* b, double* scal) {
  __shared__ double sh[256];
  double m = 0.0, sq = 0.0;
  for (int j = threadIdx.x; j < n; j += 256) {
    const double g = gs[j];
    b[j] = -g;
    const double a = fabs(g / scale[j]);
    m = (a > m || a != a) ? a : m;  // (a NaN is kept: the evaluation is reported as failed)
  }
  for (int j = threadIdx.x; j < ng; j += 256) sq += x[j] * x[j];
  sh[threadIdx.x] = m;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) { const double o = sh[threadIdx.x + w], c = sh[threadIdx.x]; sh[threadIdx.x] = (o > c || o != o) ? o : c; }
    __syncthreads();
  }
  m = sh[0];
  __syncthreads();
  sq = block_sum_256(sq, sh);
  if (threadIdx.x == 0) { scal[kCgGradMax] = m; scal[kCgXSq] = sq; }
}
void launch_cgnr_gradient_norms(const double* gs, const double* scale, int n, const double* x, int ng, double* b, double* scal, hipStream_t s) {
  hipLaunchKernelGGL(cgnr_gradient_norms_kernel, dim3(1), dim3(256), 0, s, gs, scale, n, x, ng, b, scal);
}

// ---- the preconditioner's factors -------------------------------------------------------------------------------------------------
// One lane per column block: D2 of its columns, and the Cholesky factor of its size x size matrix (size <= kCgnrMaxBlock) in the
// lane's own memory, row-major lower triangle with the diagonal.
__global__ __launch_bounds__(64) void cgnr_precond_factor_kernel(CgnrCols C, const double* bsum, double lo, double hi, double radius, double* D2, double* L, int* flags,
                                                                 const double* sub) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C.num_cb) return;
  const int size = C.cb_size[c], col = C.cb_col[c];
  const double* m = bsum + C.cb_moff[c];
  double a[kCgnrMaxBlock * kCgnrMaxBlock];
  for (int j = 0; j < size; ++j) {
    const double d = fmin(fmax(m[j * size + j], lo), hi) / radius;
    D2[col + j] = d;
    if (L) for (int k = 0; k <= j; ++k) a[j * size + k] = m[j * size + k] + (k == j ? d : 0.0);
    if (L && sub) for (int k = 0; k <= j; ++k) a[j * size + k] -= sub[C.cb_moff[c] + j * size + k];
  }
  if (!L) return;
  bool ok = true;
  for (int j = 0; j < size; ++j) {
    double d = a[j * size + j];
    for (int k = 0; k < j; ++k) d -= a[j * size + k] * a[j * size + k];
    if (cg_bad(d)) { ok = false; break; }
    d = sqrt(d);
    a[j * size + j] = d;
    for (int i = j + 1; i < size; ++i) {
      double v = a[i * size + j];
      for (int k = 0; k < j; ++k) v -= a[i * size + k] * a[j * size + k];
      a[i * size + j] = v / d;
    }
  }
  if (!ok) { flags[kCgFail] = 1; return; }
  double* out = L + C.cb_moff[c];
  for (int j = 0; j < size; ++j) for (int k = 0; k <= j; ++k) out[j * size + k] = a[j * size + k];
}
void launch_cgnr_precond_factor(const CgnrCols& C, const double* bsum, double lo, double hi, double radius, double* D2, double* L, int* flags, hipStream_t s,
                                const double* sub) {
  if (C.num_cb > 0) hipLaunchKernelGGL(cgnr_precond_factor_kernel, dim3((C.num_cb + 63) / 64), dim3(64), 0, s, C, bsum, lo, hi, radius, D2, L, flags, sub);
}

// ---- w = J v ----------------------------------------------------------------------------------------------------------------------
// One lane per row: it walks the row of its residual block's values and gathers v through the block's slots.  The direction of an
// iteration is formed where it is read, p = fma(beta, p_old, z): cgnr_jtw_kernel stores the same expression.
__global__ __launch_bounds__(256) void cgnr_jp_kernel(CgnrJac J, const double* z, const double* p, const double* scal, double* w, const int* flags) {
  if (cg_done(flags)) return;
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= J.num_rows) return;
  const double beta = p ? scal[kCgBeta] : 0.0;
  const int i = J.row_block[row], r = row - J.row_off[i];
  const int nres = J.row_off[i + 1] - J.row_off[i];
  const int width = (J.val_off[i + 1] - J.val_off[i]) / nres;
  const double* v = J.values + J.val_off[i] + (size_t)r * width;
  double s = 0.0;
  for (int slot = J.slot_begin[i]; slot < J.slot_begin[i + 1]; ++slot) {
    const int pos = J.slot_pos[slot];
    if (pos < 0) continue;
    const int col = J.slot_col[slot], size = J.slot_size[slot];
    for (int j = 0; j < size; ++j) s += v[pos + j] * (p ? fma(beta, p[col + j], z[col + j]) : z[col + j]);
  }
  w[row] = s;
}
void launch_cgnr_jp(const CgnrJac& J, const double* z, const double* p, const double* scal, double* w, const int* flags, hipStream_t s) {
  if (J.num_rows > 0) hipLaunchKernelGGL(cgnr_jp_kernel, dim3((J.num_rows + 255) / 256), dim3(256), 0, s, J, z, p, scal, w, flags);
}

// ---- q = J^T w + D2 v -------------------------------------------------------------------------------------------------------------
// A part belongs to kCgnrLanes lanes: lane l takes the part's slots l, l + kCgnrLanes, ... in plan order, then a butterfly over the
// lanes.  The only part of a block finishes it (D2 v, the store of p); the parts of a long block leave partial sums that
// cgnr_jtw_long_kernel adds the same way, lane l taking parts l, l + kCgnrLanes, ...
__device__ inline void cgnr_jtw_finish(int mode, int col, int size, const double* acc, const double* D2, const double* z, double* p, double beta, double* q) {
#pragma unroll
  for (int j = 0; j < kCgnrMaxBlock; ++j) {
    if (j >= size) continue;
    double v = acc[j];
    if (mode == kCgnrJtwCg) { const double pn = fma(beta, p[col + j], z[col + j]); p[col + j] = pn; v += D2[col + j] * pn; }
    else if (mode == kCgnrJtwVector) v += D2[col + j] * z[col + j];
    else if (mode == kCgnrJtwNegated) v = -v;
    q[col + j] = v;
  }
}
__global__ __launch_bounds__(64) void cgnr_jtw_kernel(int mode, CgnrJac J, CgnrCols C, const double* w, const double* D2, const double* z, double* p,
                                                      const double* scal, double* q, double* partial, const int* flags) {
  if (cg_done(flags)) return;
  const int sub = threadIdx.x / kCgnrLanes, lane = threadIdx.x % kCgnrLanes;
  const int part = blockIdx.x * (64 / kCgnrLanes) + sub;
  if (part >= C.num_parts) return;  // (a whole group of lanes leaves: the butterfly stays inside a group)
  const int c = C.part_cb[part], size = C.cb_size[c], begin = C.part_begin[part], end = C.part_end[part], out = C.part_out[part];
  double acc[kCgnrMaxBlock];
#pragma unroll
  for (int j = 0; j < kCgnrMaxBlock; ++j) acc[j] = 0.0;
  for (int k = begin + lane; k < end; k += kCgnrLanes) {
    const int slot = C.cb_slots[k], i = J.slot_owner[slot];
    const int row0 = J.row_off[i], nres = J.row_off[i + 1] - row0;
    const int width = (J.val_off[i + 1] - J.val_off[i]) / nres;
    const double* v = J.values + J.val_off[i] + J.slot_pos[slot];
    for (int r = 0; r < nres; ++r) {
      const double wv = w[row0 + r];
#pragma unroll
      for (int j = 0; j < kCgnrMaxBlock; ++j) if (j < size) acc[j] += v[(size_t)r * width + j] * wv;
    }
  }
#pragma unroll
  for (int j = 0; j < kCgnrMaxBlock; ++j)
    for (int off = kCgnrLanes / 2; off > 0; off >>= 1) acc[j] += __shfl_xor(acc[j], off, kCgnrLanes);
  if (lane != 0) return;
  if (out < 0) {
    cgnr_jtw_finish(mode, C.cb_col[c], size, acc, D2, z, p, mode == kCgnrJtwCg ? scal[kCgBeta] : 0.0, q);
  } else {
#pragma unroll
    for (int j = 0; j < kCgnrMaxBlock; ++j) if (j < size) partial[(size_t)out * kCgnrLanes + j] = acc[j];
  }
}
__global__ __launch_bounds__(64) void cgnr_jtw_long_kernel(int mode, CgnrCols C, const double* D2, const double* z, double* p, const double* scal, double* q,
                                                           const double* partial, const int* flags) {
  if (cg_done(flags)) return;
  const int sub = threadIdx.x / kCgnrLanes, lane = threadIdx.x % kCgnrLanes;
  const int lb = blockIdx.x * (64 / kCgnrLanes) + sub;
  if (lb >= C.num_long) return;
  const int c = C.long_cb[lb], size = C.cb_size[c], begin = C.long_begin[lb], end = C.long_begin[lb + 1];
  double acc[kCgnrMaxBlock];
#pragma unroll
  for (int j = 0; j < kCgnrMaxBlock; ++j) acc[j] = 0.0;
  for (int k = begin + lane; k < end; k += kCgnrLanes) {
#pragma unroll
    for (int j = 0; j < kCgnrMaxBlock; ++j) if (j < size) acc[j] += partial[(size_t)k * kCgnrLanes + j];
  }
#pragma unroll
  for (int j = 0; j < kCgnrMaxBlock; ++j)
    for (int off = kCgnrLanes / 2; off > 0; off >>= 1) acc[j] += __shfl_xor(acc[j], off, kCgnrLanes);
  if (lane == 0) cgnr_jtw_finish(mode, C.cb_col[c], size, acc, D2, z, p, mode == kCgnrJtwCg ? scal[kCgBeta] : 0.0, q);
}
void launch_cgnr_jtw(int mode, const CgnrJac& J, const CgnrCols& C, const double* w, const double* D2, const double* z, double* p, const double* scal,
                     double* q, double* partial, const int* flags, hipStream_t s) {
  const int per = 64 / kCgnrLanes;
  if (C.num_parts > 0) hipLaunchKernelGGL(cgnr_jtw_kernel, dim3((C.num_parts + per - 1) / per), dim3(64), 0, s, mode, J, C, w, D2, z, p, scal, q, partial, flags);
  if (C.num_long > 0) hipLaunchKernelGGL(cgnr_jtw_long_kernel, dim3((C.num_long + per - 1) / per), dim3(64), 0, s, mode, C, D2, z, p, scal, q, (const double*)partial, flags);
}

// ---- dot products -----------------------------------------------------------------------------------------------------------------
// Two stages in a fixed order, as the cost sum of Problem::Evaluate: a workgroup sums kCgnrDotChunk neighbouring terms, one
// workgroup (cgnr_sum_kernel, or a scalar kernel) sums the partial sums.
__global__ __launch_bounds__(256) void cgnr_dot_kernel(int kind, const double* a, const double* b, int n, double* partials, const int* flags) {
  __shared__ double sh[256];
  if (cg_done(flags)) return;
  const int begin = blockIdx.x * kCgnrDotChunk, end = min(n, begin + kCgnrDotChunk);
  double s = 0.0;
  for (int i = begin + threadIdx.x; i < end; i += 256) s += kind == 0 ? a[i] * b[i] : a[i] * (b[i] + 0.5 * a[i]);
  s = block_sum_256(s, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}
void launch_cgnr_dot(int kind, const double* a, const double* b, int n, double* partials, const int* flags, hipStream_t s) {
  const int nparts = (n + kCgnrDotChunk - 1) / kCgnrDotChunk;
  if (nparts > 0) hipLaunchKernelGGL(cgnr_dot_kernel, dim3(nparts), dim3(256), 0, s, kind, a, b, n, partials, flags);
}
__device__ inline double cgnr_sum_partials(const double* partials, int n, int stride, double* sh) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += partials[(size_t)i * stride];
  return block_sum_256(s, sh);
}
__global__ __launch_bounds__(256) void cgnr_sum_kernel(const double* partials, int n, double* out, const int* flags) {
  __shared__ double sh[256];
  if (cg_done(flags)) return;
  const double s = cgnr_sum_partials(partials, n, 1, sh);
  if (threadIdx.x == 0) *out = s;
}
void launch_cgnr_sum(const double* partials, int n, double* out, const int* flags, hipStream_t s) {
  hipLaunchKernelGGL(cgnr_sum_kernel, dim3(1), dim3(256), 0, s, partials, n, out, flags);
}

__global__ __launch_bounds__(256) void cgnr_axpy_kernel(const double* scal, const double* p, double* x, int n, const int* flags) {
  if (cg_done(flags)) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[i] = fma(scal[kCgAlpha], p[i], x[i]);
}
void launch_cgnr_axpy(const double* scal, const double* p, double* x, int n, const int* flags, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(cgnr_axpy_kernel, dim3((n + 255) / 256), dim3(256), 0, s, scal, p, x, n, flags);
}

// ---- the fused update -------------------------------------------------------------------------------------------------------------
// One lane per column block: the block's entries of x and res, then z = M^-1 res by two triangular solves with the block's factor,
// then the block's terms of the three dot products; the workgroup adds the terms of its kCgnrBlockChunk blocks in a fixed tree.
__global__ __launch_bounds__(256) void cgnr_update_kernel(int mode, CgnrCols C, const double* L, const double* b, const double* p, const double* q, const double* scal,
                                                          double* x, double* res, double* z, double* partials, const int* flags) {
  __shared__ double sh[256];
  if (cg_done(flags)) return;
  const int c = blockIdx.x * kCgnrBlockChunk + threadIdx.x;
  double s_rz = 0.0, s_xq = 0.0, s_bb = 0.0;
  if (c < C.num_cb) {
    const int size = C.cb_size[c], col = C.cb_col[c];
    const double alpha = mode == kCgnrStep ? scal[kCgAlpha] : 0.0;
    double rs[kCgnrMaxBlock], zz[kCgnrMaxBlock];
    for (int j = 0; j < size; ++j) {
      const double bj = b[col + j];
      double xj = x[col + j], r;
      if (mode == kCgnrInit) r = bj;
      else if (mode == kCgnrStep) { xj = fma(alpha, p[col + j], xj); x[col + j] = xj; r = fma(-alpha, q[col + j], res[col + j]); }
      else r = bj - q[col + j];
      res[col + j] = r; rs[j] = r;
      s_xq += xj * (bj + r);
      s_bb += bj * bj;
    }
    if (L) {
      const double* l = L + C.cb_moff[c];
      for (int j = 0; j < size; ++j) {  // L y = res
        double v = rs[j];
        for (int k = 0; k < j; ++k) v -= l[j * size + k] * zz[k];
        zz[j] = v / l[j * size + j];
      }
      for (int j = size - 1; j >= 0; --j) {  // L^T z = y
        double v = zz[j];
        for (int k = j + 1; k < size; ++k) v -= l[k * size + j] * zz[k];
        zz[j] = v / l[j * size + j];
      }
    } else {
      for (int j = 0; j < size; ++j) zz[j] = rs[j];
    }
    for (int j = 0; j < size; ++j) { z[col + j] = zz[j]; s_rz += rs[j] * zz[j]; }
  }
  s_rz = block_sum_256(s_rz, sh);
  s_xq = block_sum_256(s_xq, sh);
  s_bb = block_sum_256(s_bb, sh);
  if (threadIdx.x == 0) { partials[3 * blockIdx.x] = s_rz; partials[3 * blockIdx.x + 1] = s_xq; partials[3 * blockIdx.x + 2] = s_bb; }
}
void launch_cgnr_update(int mode, const CgnrCols& C, const double* L, const double* b, const double* p, const double* q, const double* scal,
                        double* x, double* res, double* z, double* partials, const int* flags, hipStream_t s) {
  static_assert(kCgnrBlockChunk == 256, "one lane per column block of the chunk");
  if (C.num_cb > 0) hipLaunchKernelGGL(cgnr_update_kernel, dim3((C.num_cb + kCgnrBlockChunk - 1) / kCgnrBlockChunk), dim3(256), 0, s, mode, C, L, b, p, q, scal, x, res, z, partials, flags);
}

// ---- the scalar kernels -----------------------------------------------------------------------------------------------------------
// One workgroup each: the second stage of the dot products before them, and the control flow of common.hpp's namespace cgnr.
__global__ __launch_bounds__(256) void cgnr_scalar_init_kernel(const double* partials3, int nparts, double* scal, int* flags) {
  __shared__ double sh[256];
  const double rho = cgnr_sum_partials(partials3, nparts, 3, sh);
  const double bb = cgnr_sum_partials(partials3 + 2, nparts, 3, sh);
  if (threadIdx.x != 0) return;
  scal[kCgRho] = rho; scal[kCgRhoLast] = 0.0; scal[kCgBeta] = 0.0; scal[kCgQ0] = 0.0; scal[kCgQ1] = 0.0; scal[kCgZeta] = 0.0; scal[kCgBb] = bb;
  scal[kCgPq] = 0.0; scal[kCgAlpha] = 0.0;
  flags[kCgIt] = 0;
  if (bb == 0.0) { flags[kCgStatus] = cgnr::kZeroRhs; flags[kCgDone] = 1; }
  else if (cg_bad(rho)) { flags[kCgStatus] = cgnr::kBreakdown; flags[kCgDone] = 1; }
  else { flags[kCgStatus] = cgnr::kRunning; flags[kCgDone] = 0; }
}
void launch_cgnr_scalar_init(const double* partials3, int nparts, double* scal, int* flags, hipStream_t s) {
  hipLaunchKernelGGL(cgnr_scalar_init_kernel, dim3(1), dim3(256), 0, s, partials3, nparts, scal, flags);
}
__global__ __launch_bounds__(256) void cgnr_scalar_alpha_kernel(const double* partials, int nparts, double* scal, int* flags) {
  __shared__ double sh[256];
  if (flags[kCgDone]) return;
  const double pq = cgnr_sum_partials(partials, nparts, 1, sh);
  if (threadIdx.x != 0) return;
  scal[kCgPq] = pq;
  if (cg_bad(pq)) { flags[kCgStatus] = cgnr::kBreakdown; flags[kCgDone] = 1; return; }
  scal[kCgAlpha] = scal[kCgRho] / pq;
}
void launch_cgnr_scalar_alpha(const double* partials, int nparts, double* scal, int* flags, hipStream_t s) {
  hipLaunchKernelGGL(cgnr_scalar_alpha_kernel, dim3(1), dim3(256), 0, s, partials, nparts, scal, flags);
}
__global__ __launch_bounds__(256) void cgnr_scalar_end_kernel(const double* partials3, int nparts, double eta, int min_it, int max_it, double* scal, int* flags) {
  __shared__ double sh[256];
  if (flags[kCgDone]) return;
  const double rho_next = cgnr_sum_partials(partials3, nparts, 3, sh);
  const double xq = cgnr_sum_partials(partials3 + 1, nparts, 3, sh);
  if (threadIdx.x != 0) return;
  const int it = flags[kCgIt] + 1;
  flags[kCgIt] = it;
  const double q1 = -0.5 * xq, q0 = scal[kCgQ0];
  const double zeta = (double)it * (q1 - q0) / q1;
  scal[kCgQ1] = q1; scal[kCgZeta] = zeta;
  if (zeta < eta && it >= min_it) { flags[kCgStatus] = cgnr::kConverged; flags[kCgDone] = 1; return; }
  scal[kCgQ0] = q1;
  if (it >= max_it) { flags[kCgStatus] = cgnr::kIterationLimit; flags[kCgDone] = 1; return; }
  const double rho = scal[kCgRho];
  scal[kCgRhoLast] = rho; scal[kCgRho] = rho_next;
  if (cg_bad(rho_next)) { flags[kCgStatus] = cgnr::kBreakdown; flags[kCgDone] = 1; return; }
  scal[kCgBeta] = rho_next / rho;
}
void launch_cgnr_scalar_end(const double* partials3, int nparts, double eta, int min_it, int max_it, double* scal, int* flags, hipStream_t s) {
  hipLaunchKernelGGL(cgnr_scalar_end_kernel, dim3(1), dim3(256), 0, s, partials3, nparts, eta, min_it, max_it, scal, flags);
}

// ---- the Schur elimination --------------------------------------------------------------------------------------------------------
// w <- w - J_e V_e^-1 J_e^T w per e-block, the hot kernel of an application of S.  t = J_e^T w is summed as cgnr_jtw_kernel sums
// it (kCgnrLanes lanes per part, the butterfly leaves the same bits in every lane); the lanes of a single-part block then each
// solve with the block's factor and subtract J_e u from the rows of their own slots.  No other e-block has entries in those rows,
// and every read of w by the group precedes the butterfly, so the stores need no atomics.  A long e-block leaves partial sums;
// cgnr_eliminate_long_kernel adds them in part order, solves and subtracts over the block's whole slot list.
__device__ inline void cgnr_eliminate_finish(int mode, const CgnrJac& J, const CgnrCols& E, int c, int begin, int end, int lane, double* t, const double* L,
                                             const double* b, double* w, double* y) {
  const int size = E.cb_size[c], col = E.cb_col[c];
  const double* l = L + E.cb_moff[c];
  if (mode == kCgnrElimBacksub) {
#pragma unroll
    for (int j = 0; j < kCgnrMaxBlock; ++j) if (j < size) t[j] = b[col + j] - t[j];
  }
#pragma unroll
  for (int j = 0; j < kCgnrMaxBlock; ++j) {  // L u' = t
    if (j >= size) continue;
    double v = t[j];
#pragma unroll
    for (int k = 0; k < j; ++k) v -= l[j * size + k] * t[k];
    t[j] = v / l[j * size + j];
  }
#pragma unroll
  for (int j = kCgnrMaxBlock - 1; j >= 0; --j) {  // L^T u = u'
    if (j >= size) continue;
    double v = t[j];
#pragma unroll
    for (int k = j + 1; k < kCgnrMaxBlock; ++k) if (k < size) v -= l[k * size + j] * t[k];
    t[j] = v / l[j * size + j];
  }
  if (mode == kCgnrElimBacksub) {
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < kCgnrMaxBlock; ++j) if (j < size) y[col + j] = t[j];
    }
    return;
  }
  for (int k = begin + lane; k < end; k += kCgnrLanes) {
    const int slot = E.cb_slots[k], i = J.slot_owner[slot];
    // a residual block that names the e-block more than once: the first of its slots subtracts for all of them (one store per row)
    bool first = true;
    for (int o = J.slot_begin[i]; o < slot; ++o) if (J.slot_pos[o] >= 0 && J.slot_col[o] == col) first = false;
    if (!first) continue;
    const int row0 = J.row_off[i], nres = J.row_off[i + 1] - row0;
    const int width = (J.val_off[i + 1] - J.val_off[i]) / nres;
    for (int r = 0; r < nres; ++r) {
      double s = 0.0;
      for (int o = slot; o < J.slot_begin[i + 1]; ++o) {
        if (J.slot_pos[o] < 0 || J.slot_col[o] != col) continue;
        const double* v = J.values + J.val_off[i] + (size_t)r * width + J.slot_pos[o];
#pragma unroll
        for (int j = 0; j < kCgnrMaxBlock; ++j) if (j < size) s += v[j] * t[j];
      }
      w[row0 + r] -= s;
    }
  }
}
__global__ __launch_bounds__(64) void cgnr_eliminate_kernel(int mode, CgnrJac J, CgnrCols E, const double* L, const double* b, double* w, double* y, double* partial,
                                                            const int* flags) {
  if (cg_done(flags)) return;
  const int sub = threadIdx.x / kCgnrLanes, lane = threadIdx.x % kCgnrLanes;
  const int part = blockIdx.x * (64 / kCgnrLanes) + sub;
  if (part >= E.num_parts) return;  // (a whole group of lanes leaves: the butterfly stays inside a group)
  const int c = E.part_cb[part], size = E.cb_size[c], begin = E.part_begin[part], end = E.part_end[part], out = E.part_out[part];
  double acc[kCgnrMaxBlock];
#pragma unroll
  for (int j = 0; j < kCgnrMaxBlock; ++j) acc[j] = 0.0;
  for (int k = begin + lane; k < end; k += kCgnrLanes) {
    const int slot = E.cb_slots[k], i = J.slot_owner[slot];
    const int row0 = J.row_off[i], nres = J.row_off[i + 1] - row0;
    const int width = (J.val_off[i + 1] - J.val_off[i]) / nres;
    const double* v = J.values + J.val_off[i] + J.slot_pos[slot];
    for (int r = 0; r < nres; ++r) {
      const double wv = w[row0 + r];
#pragma unroll
      for (int j = 0; j < kCgnrMaxBlock; ++j) if (j < size) acc[j] += v[(size_t)r * width + j] * wv;
    }
  }
#pragma unroll
  for (int j = 0; j < kCgnrMaxBlock; ++j)
    for (int off = kCgnrLanes / 2; off > 0; off >>= 1) acc[j] += __shfl_xor(acc[j], off, kCgnrLanes);
  if (out < 0) { cgnr_eliminate_finish(mode, J, E, c, begin, end, lane, acc, L, b, w, y); return; }
  if (lane != 0) return;
#pragma unroll
  for (int j = 0; j < kCgnrMaxBlock; ++j) if (j < size) partial[(size_t)out * kCgnrLanes + j] = acc[j];
}
__global__ __launch_bounds__(64) void cgnr_eliminate_long_kernel(int mode, CgnrJac J, CgnrCols E, const int* long_slots, const double* L, const double* b, double* w,
                                                                 double* y, const double* partial, const int* flags) {
  if (cg_done(flags)) return;
  const int sub = threadIdx.x / kCgnrLanes, lane = threadIdx.x % kCgnrLanes;
  const int lb = blockIdx.x * (64 / kCgnrLanes) + sub;
  if (lb >= E.num_long) return;
  const int c = E.long_cb[lb], size = E.cb_size[c], begin = E.long_begin[lb], end = E.long_begin[lb + 1];
  double acc[kCgnrMaxBlock];
#pragma unroll
  for (int j = 0; j < kCgnrMaxBlock; ++j) acc[j] = 0.0;
  for (int k = begin + lane; k < end; k += kCgnrLanes) {
#pragma unroll
    for (int j = 0; j < kCgnrMaxBlock; ++j) if (j < size) acc[j] += partial[(size_t)k * kCgnrLanes + j];
  }
#pragma unroll
  for (int j = 0; j < kCgnrMaxBlock; ++j)
    for (int off = kCgnrLanes / 2; off > 0; off >>= 1) acc[j] += __shfl_xor(acc[j], off, kCgnrLanes);
  cgnr_eliminate_finish(mode, J, E, c, long_slots[2 * lb], long_slots[2 * lb + 1], lane, acc, L, b, w, y);
}
void launch_cgnr_eliminate(int mode, const CgnrJac& J, const CgnrCols& E, const int* long_slots, const double* L, const double* b, double* w, double* y,
                           double* partial, const int* flags, hipStream_t s) {
  const int per = 64 / kCgnrLanes;
  if (E.num_parts > 0) hipLaunchKernelGGL(cgnr_eliminate_kernel, dim3((E.num_parts + per - 1) / per), dim3(64), 0, s, mode, J, E, L, b, w, y, partial, flags);
  if (E.num_long > 0) hipLaunchKernelGGL(cgnr_eliminate_long_kernel, dim3((E.num_long + per - 1) / per), dim3(64), 0, s, mode, J, E, long_slots, L, b, w, y, (const double*)partial, flags);
}

// The block diagonal of S, once per linear solve.  One wave per part of an F block's pair list, as cgnr_block_diag_kernel: lane e
// (e, e + 64, ... below size^2) owns entry (a, b) and walks the part's pairs in plan order.  Per pair it forms rows a and b of
// W_ge over the pair's terms, solves both with L_e and adds their product: redundant across the lanes of a row, but without a
// hand-over between lanes, and the launch runs once where the projection runs every iteration.
__global__ __launch_bounds__(64) void cgnr_schur_diag_kernel(CgnrJac J, CgnrCols F, CgnrPairs P, const double* L, double* sdiag, double* partial) {
  const int part = blockIdx.x;
  const int g = P.part_f[part], size = F.cb_size[g], begin = P.part_begin[part], end = P.part_end[part], out = P.part_out[part];
  for (int e = threadIdx.x; e < size * size; e += 64) {
    const int a = e / size, b = e - a * size;
    double s = 0.0;
    for (int q = begin; q < end; ++q) {
      const int ce = P.pair_e[q], se = P.cb_size[ce];
      const double* l = L + P.cb_moff[ce];
      double xa[kCgnrMaxBlock], xb[kCgnrMaxBlock];
#pragma unroll
      for (int j = 0; j < kCgnrMaxBlock; ++j) xa[j] = xb[j] = 0.0;
      for (int k = P.pair_slot_begin[q]; k < P.pair_slot_begin[q + 1]; ++k) {
        const int sg = P.slot_g[k], sl = P.slot_e[k], i = J.slot_owner[sg];
        const int nres = J.row_off[i + 1] - J.row_off[i];
        const int width = (J.val_off[i + 1] - J.val_off[i]) / nres;
        const double* vg = J.values + J.val_off[i] + J.slot_pos[sg];
        const double* ve = J.values + J.val_off[i] + J.slot_pos[sl];
        for (int r = 0; r < nres; ++r) {
          const double ga = vg[(size_t)r * width + a], gb = vg[(size_t)r * width + b];
#pragma unroll
          for (int j = 0; j < kCgnrMaxBlock; ++j) if (j < se) { const double ev = ve[(size_t)r * width + j]; xa[j] += ev * ga; xb[j] += ev * gb; }
        }
      }
#pragma unroll
      for (int j = 0; j < kCgnrMaxBlock; ++j) {  // L_e x = W_ge's row, twice
        if (j >= se) continue;
        double va = xa[j], vb = xb[j];
#pragma unroll
        for (int k = 0; k < j; ++k) { va -= l[j * se + k] * xa[k]; vb -= l[j * se + k] * xb[k]; }
        xa[j] = va / l[j * se + j]; xb[j] = vb / l[j * se + j];
        s += xa[j] * xb[j];
      }
    }
    if (out < 0) sdiag[F.cb_moff[g] + e] = s; else partial[(size_t)out * 256 + e] = s;
  }
}
__global__ __launch_bounds__(64) void cgnr_schur_diag_long_kernel(CgnrCols F, CgnrPairs P, double* sdiag, const double* partial) {
  const int g = P.long_f[blockIdx.x], size = F.cb_size[g];
  const int begin = P.long_begin[blockIdx.x], end = P.long_begin[blockIdx.x + 1];
  for (int e = threadIdx.x; e < size * size; e += 64) {
    double s = 0.0;
    for (int k = begin; k < end; ++k) s += partial[(size_t)k * 256 + e];
    sdiag[F.cb_moff[g] + e] = s;
  }
}
void launch_cgnr_schur_diag(const CgnrJac& J, const CgnrCols& F, const CgnrPairs& P, const double* L, double* sdiag, double* partial, hipStream_t s) {
  if (P.num_parts > 0) hipLaunchKernelGGL(cgnr_schur_diag_kernel, dim3(P.num_parts), dim3(64), 0, s, J, F, P, L, sdiag, partial);
  if (P.num_long > 0) hipLaunchKernelGGL(cgnr_schur_diag_long_kernel, dim3(P.num_long), dim3(64), 0, s, F, P, sdiag, (const double*)partial);
}

// ---- the candidate ----------------------------------------------------------------------------------------------------------------
// One lane per parameter block of the problem: x_new = x (+) delta with delta = y scale in the block's tangent space; a constant
// block is copied.
__global__ __launch_bounds__(256) void cgnr_candidate_kernel(const ParamBlock* pblocks, int num_pb, const double* y, const double* scale, const double* x, double* x_new, double* partials) {
  __shared__ double sh[256];
  const int b = blockIdx.x * 256 + threadIdx.x;
  double sq = 0.0;
  if (b < num_pb) {
    const ParamBlock pb = pblocks[b];
    const double* xb = x + pb.global_off;
    double* out = x_new + pb.global_off;
    if (pb.type == kParamConstant || pb.local_size == 0) {
      for (int i = 0; i < pb.global_size; ++i) out[i] = xb[i];
    } else {
      double delta[kParamMaxSize], xp[kParamMaxSize];
      for (int j = 0; j < pb.local_size; ++j) delta[j] = y[pb.local_off + j] * scale[pb.local_off + j];
      param_plus(pb, xb, delta, xp);
      for (int i = 0; i < pb.global_size; ++i) { out[i] = xp[i]; const double d = xb[i] - xp[i]; sq += d * d; }
    }
  }
  sq = block_sum_256(sq, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = sq;
}
void launch_cgnr_candidate(const ParamBlock* pblocks, int num_pb, const double* y, const double* scale, const double* x, double* x_new, double* partials, hipStream_t s) {
  if (num_pb > 0) hipLaunchKernelGGL(cgnr_candidate_kernel, dim3((num_pb + 255) / 256), dim3(256), 0, s, pblocks, num_pb, y, scale, x, x_new, partials);
}

}  // namespace sk
