// HIP kernels of Problem::Evaluate (sk_problem_evaluate; plan: evaluate_plan.hpp): evaluation into per-group staging planes,
// the finish (loss correction, projection into the tangent space, scatter into the caller's row order), the gradient in a
// fixed summation order and the cost.  Nothing here is scaled: these are the Jacobian and the residuals the caller asked for,
// not the solvers' (dense_kernels.hip, bal_kernels.hip).
#include <hip/hip_runtime.h>
#include "evaluate_kernels.hpp"
#include "functors.hpp"
#include "parameterization.hpp"

namespace sk {

// ---- evaluation -------------------------------------------------------------------------------------------------------------------
// One lane per residual block of functor F, as dense_eval_kernel: T = double, or Jet<sum N(i)> seeded in block order.  Entry e of
// lane l goes to stage[e * count + l]: the lanes of a wave store 64 neighbouring doubles of one plane.
template <class F, bool kJac>
__global__ void evaluate_eval_kernel(EvaluateEvalArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.count) return;
  const int b = a.blocks[a.members[i]];
  const double* c = a.consts + a.const_off[b];
  const int* xoff = a.xoff + a.pidx_off[b];
  double* out_plane = a.stage + i;
  const size_t n = (size_t)a.count;
  if (!kJac) {
    double store[F::kDim];
    const double* params[F::kBlocks];
    int k = 0;
#pragma unroll
    for (int q = 0; q < F::kBlocks; ++q) {
      params[q] = &store[k];
      const double* src = a.x + xoff[q];
      for (int j = 0; j < F::N(q); ++j) store[k++] = src[j];
    }
    double out[F::kRes];
    if (!F::template apply<double>(c, params, out)) { *a.fail_flag = 1; return; }
#pragma unroll
    for (int r = 0; r < F::kRes; ++r) out_plane[(size_t)r * n] = out[r];
  } else {
    typedef Jet<F::kDim> J;
    J store[F::kDim];
    const J* params[F::kBlocks];
    int k = 0;
#pragma unroll
    for (int q = 0; q < F::kBlocks; ++q) {
      params[q] = &store[k];
      const double* src = a.x + xoff[q];
      for (int j = 0; j < F::N(q); ++j) { store[k] = J(src[j], k); ++k; }
    }
    J out[F::kRes];
    if (!F::template apply<J>(c, params, out)) { *a.fail_flag = 1; return; }
#pragma unroll
    for (int r = 0; r < F::kRes; ++r) {
      out_plane[(size_t)r * n] = out[r].a;
#pragma unroll
      for (int d = 0; d < F::kDim; ++d) out_plane[(size_t)(F::kRes + r * F::kDim + d) * n] = out[r].v[d];
    }
  }
}

void launch_evaluate_eval(int functor_id, bool jac, const EvaluateEvalArgs& a, hipStream_t s) {
  if (a.count <= 0) return;
  const dim3 g((a.count + 127) / 128), b(128);
#define SK_LAUNCH(F)                                                               \
  do {                                                                             \
    if (jac) hipLaunchKernelGGL((evaluate_eval_kernel<F, true>), g, b, 0, s, a);   \
    else hipLaunchKernelGGL((evaluate_eval_kernel<F, false>), g, b, 0, s, a);      \
  } while (0)
  SK_DISPATCH_FUNCTOR(functor_id, SK_LAUNCH)
#undef SK_LAUNCH
}

// Recorded functors, as dense_eval_tape_kernel: W = 0 residuals only, else ceil(dim / W) passes of Jet<W>; the register files
// of the workgroup's threads in dynamic LDS.
template <int W>
__global__ void evaluate_eval_tape_kernel(EvaluateEvalArgs a, TapeDev t) {
  extern __shared__ __attribute__((aligned(16))) double tape_lds[];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.count) return;
  const int b = a.blocks[a.members[i]];
  const double* c = a.consts + a.const_off[b];
  const int* xoff = a.xoff + a.pidx_off[b];
  double* out_plane = a.stage + i;
  const size_t n = (size_t)a.count;
  auto param = [&](int k) { return a.x[xoff[t.param_block[k]] + t.param_index[k]]; };
  if (W == 0) {
    const TapeRegs<double> regs{tape_lds, (int)blockDim.x, (int)threadIdx.x};
    double out[kTapeMaxResiduals];
    tape_run<double>(t, c, param, 0, regs, out);
    for (int r = 0; r < t.num_residuals; ++r) out_plane[(size_t)r * n] = out[r];
  } else {
    typedef Jet<(W > 0 ? W : 1)> J;
    const TapeRegs<J> regs{tape_lds, (int)blockDim.x, (int)threadIdx.x};
    J out[kTapeMaxResiduals];
    for (int first = 0; first < t.dim; first += W) {
      tape_run<J>(t, c, param, first, regs, out);
      if (first == 0) for (int r = 0; r < t.num_residuals; ++r) out_plane[(size_t)r * n] = out[r].a;
      for (int w = 0; w < W && first + w < t.dim; ++w)
        for (int r = 0; r < t.num_residuals; ++r) out_plane[(size_t)(t.num_residuals + r * t.dim + first + w) * n] = out[r].v[w];
    }
  }
}

template <class K>
static void evaluate_allow_lds(K kernel, size_t bytes) {
  if (bytes > 48 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
bool launch_evaluate_eval_tape(const TapeDevBuffers& tb, bool jac, const EvaluateEvalArgs& a, hipStream_t s) {
  if (a.count <= 0) return true;
  const int threads = 128;
  const dim3 g((a.count + threads - 1) / threads), b(threads);
  if (!jac) {
    const size_t lds = tape_lds_bytes(tb.host, 0, threads);
    if (lds > kTapeLdsBudget) return false;
    evaluate_allow_lds(evaluate_eval_tape_kernel<0>, lds);
    hipLaunchKernelGGL(evaluate_eval_tape_kernel<0>, g, b, lds, s, a, tb.view);
    return true;
  }
  const int W = tape_pick_width(tb.host, threads);
  const size_t lds = tape_lds_bytes(tb.host, W, threads);
  switch (W) {
    case 3: evaluate_allow_lds(evaluate_eval_tape_kernel<3>, lds); hipLaunchKernelGGL(evaluate_eval_tape_kernel<3>, g, b, lds, s, a, tb.view); return true;
    case 2: evaluate_allow_lds(evaluate_eval_tape_kernel<2>, lds); hipLaunchKernelGGL(evaluate_eval_tape_kernel<2>, g, b, lds, s, a, tb.view); return true;
    case 1: evaluate_allow_lds(evaluate_eval_tape_kernel<1>, lds); hipLaunchKernelGGL(evaluate_eval_tape_kernel<1>, g, b, lds, s, a, tb.view); return true;
    default: return false;
  }
}

// ---- finish -----------------------------------------------------------------------------------------------------------------------
// A workgroup takes kFinishBlocks neighbouring residual blocks of the list.  Their values are ONE run of values[] (evaluate_plan.hpp),
// so after one lane per block has done the block's loss (residuals, cost term, the corrector's two scalars), the workgroup's threads
// walk that run entry by entry: neighbouring threads store neighbouring doubles, whole rows whatever the block shape, and each
// entry is computed where it is stored — corrected as LossCorrector says, then projected through param_jacobian.
constexpr int kFinishBlocks = 64, kFinishThreads = 256;

__global__ __launch_bounds__(kFinishThreads) void evaluate_finish_kernel(EvaluateFinishArgs a) {
  __shared__ int first_value[kFinishBlocks + 1];
  __shared__ double sqrt_rho1[kFinishBlocks], alpha_sq_norm[kFinishBlocks];
  const int i0 = blockIdx.x * kFinishBlocks;
  const int nblk = min(kFinishBlocks, a.num_blocks - i0);
  const int t = threadIdx.x;
  if (t <= nblk) first_value[t] = a.val_off[i0 + t];
  if (t < nblk) {
    const int i = i0 + t;
    const int row0 = a.row_off[i], nres = a.row_off[i + 1] - row0;
    const double* st = a.stage + a.blk_stage[i];
    const size_t stride = (size_t)a.blk_stride[i];
    double s = 0.0;
    for (int r = 0; r < nres; ++r) { const double v = st[r * stride]; s += v * v; }
    const int root = a.blk_loss[i];
    double scaling = 1.0;
    if (root < 0) {
      a.cterm[i] = s; sqrt_rho1[t] = 1.0; alpha_sq_norm[t] = 0.0;
    } else {
      double rho[3];
      loss_evaluate(a.nodes, root, s, rho);
      const LossCorrector c(s, rho);
      a.cterm[i] = rho[0]; sqrt_rho1[t] = c.sqrt_rho1; alpha_sq_norm[t] = c.alpha_sq_norm; scaling = c.residual_scaling;
    }
    for (int r = 0; r < nres; ++r) a.residuals[row0 + r] = root < 0 ? st[r * stride] : scaling * st[r * stride];
  }
  if (!a.values) return;
  __syncthreads();
  const int end = first_value[nblk];
  for (int e = first_value[0] + t; e < end; e += kFinishThreads) {
    int lo = 0, hi = nblk;  // the last block whose first value is <= e (blocks without values share their successor's)
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (first_value[mid] <= e) lo = mid; else hi = mid; }
    const int i = i0 + lo;
    const int nres = a.row_off[i + 1] - a.row_off[i];
    const int width = (first_value[lo + 1] - first_value[lo]) / nres;
    const int local = e - first_value[lo], r = local / width, c = local - r * width;
    int slot = a.slot_begin[i];
    const int slot_end = a.slot_begin[i + 1];
    ParamBlock pb;
    for (; slot < slot_end; ++slot) {  // (c < width: one of the stored slots holds it)
      const int pos = a.slot_pos[slot];
      if (pos < 0) continue;
      pb = a.pblocks[a.slot_block[slot]];
      if (c >= pos && c < pos + pb.local_size) break;
    }
    if (slot == slot_end) continue;
    const int j = c - a.slot_pos[slot], k0 = a.slot_k0[slot], dim = a.blk_dim[i];
    const double* st = a.stage + a.blk_stage[i];
    const size_t stride = (size_t)a.blk_stride[i];
    const double srho = sqrt_rho1[lo], alpha = alpha_sq_norm[lo];
    // corrected entry (r, g) of the block's global-size Jacobian
    auto corrected = [&](int g) -> double {
      double v = st[(size_t)(nres + r * dim + k0 + g) * stride];
      if (alpha != 0.0) {
        double rtj = 0.0;
        for (int q = 0; q < nres; ++q) rtj += st[q * stride] * st[(size_t)(nres + q * dim + k0 + g) * stride];
        v -= alpha * st[r * stride] * rtj;
      }
      return srho * v;
    };
    double v;
    if (pb.type == kParamQuaternion || pb.type == kParamHomogeneousVector) {
      double P[kParamMaxSize * kParamMaxSize];
      param_jacobian(pb, a.x + pb.global_off, P);
      v = 0.0;
      for (int g = 0; g < pb.global_size; ++g) v += corrected(g) * P[g * pb.local_size + j];
    } else if (pb.type == kParamSubset) {  // a column selection: the j-th coordinate that is not held
      int g = 0;
      for (int seen = -1; g < pb.global_size; ++g) if (!((pb.constant_mask >> g) & 1u) && ++seen == j) break;
      v = corrected(g);
    } else {
      v = corrected(j);
    }
    a.values[e] = v;
  }
}
void launch_evaluate_finish(const EvaluateFinishArgs& a, hipStream_t s) {
  if (a.num_blocks > 0) hipLaunchKernelGGL(evaluate_finish_kernel, dim3((a.num_blocks + kFinishBlocks - 1) / kFinishBlocks), dim3(kFinishThreads), 0, s, a);
}

// ---- gradient ---------------------------------------------------------------------------------------------------------------------
// g = J^T r of the values and residuals just written.  A column block belongs to kGradLanes lanes of a wave: lane l takes terms
// l, l + kGradLanes, ... of the block's list in plan order, then a butterfly over the kGradLanes lanes — the same shape of sum for
// the same plan, no atomics.  (A point with 5 observations keeps 5 lanes busy, a camera with 400 gives each lane 25 terms.)
constexpr int kGradLanes = 16, kGradThreads = 64, kGradCols = 16;

__global__ __launch_bounds__(kGradThreads) void evaluate_gradient_kernel(EvaluateGradientArgs a) {
  const int part = threadIdx.x / kGradLanes, lane = threadIdx.x % kGradLanes;
  const int cb = blockIdx.x * (kGradThreads / kGradLanes) + part;
  if (cb >= a.num_column_blocks) return;  // (a whole part leaves: the butterfly stays inside a part)
  const int col = a.grad_col[cb], size = a.grad_size[cb];
  const int begin = a.grad_begin[cb], end = a.grad_begin[cb + 1];
  for (int j0 = 0; j0 < size; j0 += kGradCols) {  // (blocks wider than kGradCols columns: callbacks, ten-parameter functors)
    const int nj = min(kGradCols, size - j0);
    double acc[kGradCols];
#pragma unroll
    for (int j = 0; j < kGradCols; ++j) acc[j] = 0.0;
    for (int e = begin + lane; e < end; e += kGradLanes) {
      const int slot = a.grad_slots[e], i = a.slot_owner[slot];
      const int row0 = a.row_off[i], nres = a.row_off[i + 1] - row0;
      const int width = (a.val_off[i + 1] - a.val_off[i]) / nres;
      const double* v = a.values + a.val_off[i] + a.slot_pos[slot] + j0;
      for (int r = 0; r < nres; ++r) {
        const double rv = a.residuals[row0 + r];
#pragma unroll
        for (int j = 0; j < kGradCols; ++j) if (j < nj) acc[j] += v[(size_t)r * width + j] * rv;
      }
    }
#pragma unroll
    for (int j = 0; j < kGradCols; ++j)
      for (int off = kGradLanes / 2; off > 0; off >>= 1) acc[j] += __shfl_xor(acc[j], off, kGradLanes);
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < kGradCols; ++j) if (j < nj) a.gradient[col + j0 + j] = acc[j];
    }
  }
}
void launch_evaluate_gradient(const EvaluateGradientArgs& a, hipStream_t s) {
  const int per = kGradThreads / kGradLanes;
  if (a.num_column_blocks > 0) hipLaunchKernelGGL(evaluate_gradient_kernel, dim3((a.num_column_blocks + per - 1) / per), dim3(kGradThreads), 0, s, a);
}

// ---- cost -------------------------------------------------------------------------------------------------------------------------
// Two stages in a fixed order: a workgroup sums kEvaluateSumChunk neighbouring terms, one workgroup sums the partial sums.
__global__ __launch_bounds__(256) void evaluate_sum_kernel(const double* v, int n, int chunk, double scale, double* out) {
  __shared__ double sh[256];
  const int begin = blockIdx.x * chunk, end = min(n, begin + chunk);
  double s = 0.0;
  for (int i = begin + threadIdx.x; i < end; i += 256) s += v[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) { if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w]; __syncthreads(); }
  if (threadIdx.x == 0) out[blockIdx.x] = scale * sh[0];
}
void launch_evaluate_cost(const double* cterm, int n, double* partials, double* cost, hipStream_t s) {
  const int nparts = (n + kEvaluateSumChunk - 1) / kEvaluateSumChunk;
  if (nparts > 0) hipLaunchKernelGGL(evaluate_sum_kernel, dim3(nparts), dim3(256), 0, s, cterm, n, kEvaluateSumChunk, 1.0, partials);
  hipLaunchKernelGGL(evaluate_sum_kernel, dim3(1), dim3(256), 0, s, (const double*)partials, nparts, max(nparts, 1), 0.5, cost);
}

}  // namespace sk
