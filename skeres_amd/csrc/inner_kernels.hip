// HIP kernels of the inner iterations (gfx950, wave64, fp64): per block of a group the sum of its cost terms, one
// Levenberg-Marquardt step in one lane (the damped normal matrix of a block is at most 16 x 16: its Cholesky factor and the two
// triangular solves stay in the lane), and the acceptance of the step.  Every kernel returns at once when the group's done flag
// is set and for a block whose solve has ended, so the host may enqueue rounds ahead.  Sums run in the plan's order; the only
// atomic is the integer count of the blocks still running.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "inner_kernels.hpp"

namespace sk {

namespace {

constexpr int kN = kParamMaxSize;           // a block's tangent size is at most this
constexpr int kTri = kN * (kN + 1) / 2;     // its lower triangle, packed by rows
#define SK_TRI(i, j) ((i) * ((i) + 1) / 2 + (j))

__device__ inline bool in_done(const int* flags) { return flags[kInDone] != 0; }

}  // namespace

// ---- begin ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void inner_begin_kernel(InnerGroupDev G, InnerDev D) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e == 0) { D.flags[kInRounds] = 0; D.flags[kInDone] = 0; D.flags[kInActive] = 0; }
  if (e >= G.cols.num_cb) return;
  const int pb = G.pb[e];
  double* st = D.st + (size_t)pb * kInDCount;
  int* sti = D.sti + (size_t)pb * kInICount;
  st[kInRadius] = inner::kInitialRadius; st[kInDecrease] = 2.0; st[kInCost] = 0.0; st[kInModel] = 0.0; st[kInStepNorm] = 0.0; st[kInXNorm] = 0.0;
  sti[kInStatus] = inner::kRunning; sti[kInIters] = 0; sti[kInInvalid] = 0; sti[kInTried] = 0; sti[kInScaled] = 0;
}
void launch_inner_begin(const InnerGroupDev& G, const InnerDev& D, hipStream_t s) {
  hipLaunchKernelGGL(inner_begin_kernel, dim3((G.cols.num_cb + 255) / 256 > 0 ? (G.cols.num_cb + 255) / 256 : 1), dim3(256), 0, s, G, D);
}

// ---- a block's cost ---------------------------------------------------------------------------------------------------------------
// As cgnr_jtw_kernel: a part belongs to kCgnrLanes lanes, lane l takes the part's entries l, l + kCgnrLanes, ..., then a butterfly
// over the lanes; the parts of a long block leave partial sums that the second launch adds the same way.
__global__ __launch_bounds__(64) void inner_cost_kernel(InnerGroupDev G, InnerDev D, const double* cterm, double* out_sum) {
  if (in_done(D.flags)) return;
  const int sub = threadIdx.x / kCgnrLanes, lane = threadIdx.x % kCgnrLanes;
  const int part = blockIdx.x * (64 / kCgnrLanes) + sub;
  if (part >= G.cols.num_parts) return;  // (a whole group of lanes leaves: the butterfly stays inside a group)
  const int e = G.cols.part_cb[part];
  if (D.sti[(size_t)G.pb[e] * kInICount + kInStatus] != inner::kRunning) return;
  const int begin = G.cols.part_begin[part], end = G.cols.part_end[part], out = G.cols.part_out[part];
  double acc = 0.0;
  for (int k = begin + lane; k < end; k += kCgnrLanes) { const int i = G.cost_rb[k]; if (i >= 0) acc += cterm[i]; }
  for (int off = kCgnrLanes / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, kCgnrLanes);
  if (lane != 0) return;
  if (out < 0) out_sum[e] = acc; else D.cost_partial[out] = acc;
}
__global__ __launch_bounds__(64) void inner_cost_long_kernel(InnerGroupDev G, InnerDev D, double* out_sum) {
  if (in_done(D.flags)) return;
  const int sub = threadIdx.x / kCgnrLanes, lane = threadIdx.x % kCgnrLanes;
  const int lb = blockIdx.x * (64 / kCgnrLanes) + sub;
  if (lb >= G.cols.num_long) return;
  const int e = G.cols.long_cb[lb];
  if (D.sti[(size_t)G.pb[e] * kInICount + kInStatus] != inner::kRunning) return;
  double acc = 0.0;
  for (int k = G.cols.long_begin[lb] + lane; k < G.cols.long_begin[lb + 1]; k += kCgnrLanes) acc += D.cost_partial[k];
  for (int off = kCgnrLanes / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, kCgnrLanes);
  if (lane == 0) out_sum[e] = acc;
}
void launch_inner_cost(const InnerGroupDev& G, const InnerDev& D, const double* cterm, double* out, hipStream_t s) {
  const int per = 64 / kCgnrLanes;
  if (G.cols.num_parts > 0) hipLaunchKernelGGL(inner_cost_kernel, dim3((G.cols.num_parts + per - 1) / per), dim3(64), 0, s, G, D, cterm, out);
  if (G.cols.num_long > 0) hipLaunchKernelGGL(inner_cost_long_kernel, dim3((G.cols.num_long + per - 1) / per), dim3(64), 0, s, G, D, out);
}

// ---- the step ---------------------------------------------------------------------------------------------------------------------
// One lane per block.  The matrix is held as a 16 x 16 lower triangle whatever the block's size, padded with the identity: every
// index is a compile-time constant, and the entries of the block itself see the operations of an unpadded factorisation.
__global__ __launch_bounds__(64) void inner_step_kernel(InnerGroupDev G, InnerDev D, const ParamBlock* pblocks, const double* x, double* xc) {
  if (in_done(D.flags)) return;
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= G.cols.num_cb) return;
  const int pbi = G.pb[e];
  double* st = D.st + (size_t)pbi * kInDCount;
  int* sti = D.sti + (size_t)pbi * kInICount;
  if (sti[kInStatus] != inner::kRunning) return;
  const int size = G.cols.cb_size[e], col = G.cols.cb_col[e];
  const double* H = D.H + G.cols.cb_moff[e];
  const double cost = 0.5 * D.csum[e];
  st[kInCost] = cost;
  sti[kInTried] = 0;
  if (!sti[kInScaled]) {
    for (int j = 0; j < size; ++j) D.scale[col + j] = 1.0 / (1.0 + sqrt(H[j * size + j]));
    sti[kInScaled] = 1;
  }
  // FinalizeIterationAndCheckIfMinimizerCanContinue, as SolverBase::step
  double gmax = 0.0;
  for (int j = 0; j < size; ++j) { const double a = fabs(D.g[col + j]); gmax = (a > gmax || a != a) ? a : gmax; }
  if (sti[kInIters] >= inner::kMaxNumIterations) { sti[kInStatus] = inner::kIterationLimit; return; }
  if (gmax <= inner::kGradientTolerance) { sti[kInStatus] = inner::kGradient; return; }
  const double radius = st[kInRadius];
  if (radius < inner::kMinRadius) { sti[kInStatus] = inner::kRadius; return; }
  sti[kInIters] += 1;

  double sc[kN], gs[kN], a[kTri];
#pragma unroll
  for (int j = 0; j < kN; ++j) { sc[j] = j < size ? D.scale[col + j] : 0.0; gs[j] = j < size ? D.g[col + j] * sc[j] : 0.0; }
#pragma unroll
  for (int j = 0; j < kN; ++j) {
#pragma unroll
    for (int k = 0; k <= j; ++k) {
      double v = k == j ? 1.0 : 0.0;
      if (j < size) {
        v = H[j * size + k] * sc[j] * sc[k];
        if (k == j) v += fmin(fmax(v, inner::kMinLmDiagonal), inner::kMaxLmDiagonal) / radius;
      }
      a[SK_TRI(j, k)] = v;
    }
  }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < kN; ++j) {
    double d = a[SK_TRI(j, j)];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= a[SK_TRI(j, k)] * a[SK_TRI(j, k)];
    if (!(d > 0.0) || !isfinite(d)) { ok = false; d = 1.0; }
    d = sqrt(d);
    a[SK_TRI(j, j)] = d;
#pragma unroll
    for (int i = j + 1; i < kN; ++i) {
      double v = a[SK_TRI(i, j)];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= a[SK_TRI(i, k)] * a[SK_TRI(j, k)];
      a[SK_TRI(i, j)] = v / d;
    }
  }
  double y[kN];
#pragma unroll
  for (int j = 0; j < kN; ++j) {  // L t = gs
    double v = gs[j];
#pragma unroll
    for (int k = 0; k < j; ++k) v -= a[SK_TRI(j, k)] * y[k];
    y[j] = v / a[SK_TRI(j, j)];
  }
#pragma unroll
  for (int j = kN - 1; j >= 0; --j) {  // L^T u = t
    double v = y[j];
#pragma unroll
    for (int k = j + 1; k < kN; ++k) v -= a[SK_TRI(k, j)] * y[k];
    y[j] = v / a[SK_TRI(j, j)];
  }
#pragma unroll
  for (int j = 0; j < kN; ++j) y[j] = -y[j];
  // the model's change -(y . gs + y^T Hs y / 2), Hs read again: the factor has replaced it
  double yg = 0.0, yhy = 0.0;
#pragma unroll
  for (int j = 0; j < kN; ++j) {
    if (j >= size) continue;
    yg += y[j] * gs[j];
    double w = 0.0;
#pragma unroll
    for (int k = 0; k < kN; ++k) if (k < size) w += H[j * size + k] * sc[j] * sc[k] * y[k];
    yhy += y[j] * w;
  }
  const double model = -(yg + 0.5 * yhy);
  const ParamBlock pb = pblocks[pbi];
  const double* xb = x + pb.global_off;
  double delta[kN], xp[kN];
#pragma unroll
  for (int j = 0; j < kN; ++j) { delta[j] = y[j] * sc[j]; xp[j] = 0.0; }
  param_plus(pb, xb, delta, xp);
  double dsq = 0.0, xsq = 0.0;
  bool finite = isfinite(model);
  for (int i = 0; i < pb.global_size; ++i) { const double d = xb[i] - xp[i]; dsq += d * d; xsq += xb[i] * xb[i]; finite = finite && isfinite(xp[i]); }
  if (!ok || !finite || !(model > 0.0)) {  // an invalid step: StepIsInvalid == StepRejected
    const int invalid = sti[kInInvalid] + 1;
    sti[kInInvalid] = invalid;
    if (invalid >= inner::kMaxConsecutiveInvalidSteps) { sti[kInStatus] = inner::kInvalidSteps; return; }
    const double df = st[kInDecrease];
    st[kInRadius] = radius / df; st[kInDecrease] = 2.0 * df;
    return;
  }
  sti[kInTried] = 1;
  st[kInModel] = model; st[kInStepNorm] = sqrt(dsq); st[kInXNorm] = sqrt(xsq);
  double* out = xc + pb.global_off;
  for (int i = 0; i < pb.global_size; ++i) out[i] = xp[i];
}
void launch_inner_step(const InnerGroupDev& G, const InnerDev& D, const ParamBlock* pblocks, const double* x, double* xc, hipStream_t s) {
  if (G.cols.num_cb > 0) hipLaunchKernelGGL(inner_step_kernel, dim3((G.cols.num_cb + 63) / 64), dim3(64), 0, s, G, D, pblocks, x, xc);
}

// ---- acceptance -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void inner_accept_kernel(InnerGroupDev G, InnerDev D, const ParamBlock* pblocks, double* x, double* xc) {
  if (in_done(D.flags)) return;
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= G.cols.num_cb) return;
  const int pbi = G.pb[e];
  double* st = D.st + (size_t)pbi * kInDCount;
  int* sti = D.sti + (size_t)pbi * kInICount;
  if (sti[kInStatus] != inner::kRunning) return;
  if (sti[kInTried]) {
    sti[kInTried] = 0; sti[kInInvalid] = 0;
    const double cost = st[kInCost], model = st[kInModel], step_norm = st[kInStepNorm], radius = st[kInRadius];
    double new_cost = 0.5 * D.csum_c[e];
    if (!isfinite(new_cost)) new_cost = DBL_MAX;
    const double cost_change = cost - new_cost;
    bool accept = false;
    if (step_norm <= inner::kParameterTolerance * (st[kInXNorm] + inner::kParameterTolerance)) {
      sti[kInStatus] = inner::kParameter;
    } else if (fabs(cost_change) <= inner::kFunctionTolerance * cost) {
      sti[kInStatus] = inner::kFunction;
    } else {
      const double rho = cost_change / model;
      if (rho > inner::kMinRelativeDecrease) {
        accept = true;
        const double t = 2.0 * rho - 1.0;
        st[kInRadius] = fmin(inner::kMaxRadius, radius / fmax(1.0 / 3.0, 1.0 - t * t * t));
        st[kInDecrease] = 2.0;
      } else {
        const double df = st[kInDecrease];
        st[kInRadius] = radius / df; st[kInDecrease] = 2.0 * df;
      }
    }
    const ParamBlock pb = pblocks[pbi];
    double* xb = x + pb.global_off;
    double* cb = xc + pb.global_off;
    for (int i = 0; i < pb.global_size; ++i) { if (accept) xb[i] = cb[i]; else cb[i] = xb[i]; }
  }
  if (sti[kInStatus] == inner::kRunning) atomicAdd(&D.flags[kInActive], 1);
}
void launch_inner_accept(const InnerGroupDev& G, const InnerDev& D, const ParamBlock* pblocks, double* x, double* xc, hipStream_t s) {
  if (G.cols.num_cb > 0) hipLaunchKernelGGL(inner_accept_kernel, dim3((G.cols.num_cb + 63) / 64), dim3(64), 0, s, G, D, pblocks, x, xc);
}

__global__ __launch_bounds__(64) void inner_round_end_kernel(InnerDev D) {
  if (threadIdx.x != 0 || in_done(D.flags)) return;
  D.flags[kInRounds] += 1;
  if (D.flags[kInActive] == 0) D.flags[kInDone] = 1;
  D.flags[kInActive] = 0;
}
void launch_inner_round_end(const InnerDev& D, hipStream_t s) { hipLaunchKernelGGL(inner_round_end_kernel, dim3(1), dim3(64), 0, s, D); }

// ---- |a - b|^2 --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void inner_diff_sq_kernel(const double* a, const double* b, int n, double* partials) {
  __shared__ double sh[256];
  const int begin = blockIdx.x * kCgnrDotChunk, end = min(n, begin + kCgnrDotChunk);
  double s = 0.0;
  for (int i = begin + threadIdx.x; i < end; i += 256) { const double d = a[i] - b[i]; s += d * d; }
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) { if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w]; __syncthreads(); }
  if (threadIdx.x == 0) partials[blockIdx.x] = sh[0];
}
void launch_inner_diff_sq(const double* a, const double* b, int n, double* partials, hipStream_t s) {
  const int nparts = (n + kCgnrDotChunk - 1) / kCgnrDotChunk;
  if (nparts > 0) hipLaunchKernelGGL(inner_diff_sq_kernel, dim3(nparts), dim3(256), 0, s, a, b, n, partials);
}

}  // namespace sk
