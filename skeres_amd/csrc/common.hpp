// Shared host-side helpers: error reporting across the C ABI, device buffers,
// and the host mirror of Problem / CostFunction / Options / Summary.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/skeres_amd.h"
#include "dev_knobs.hpp"
#include "functors.hpp"
#include "loss.hpp"
#include "parameterization.hpp"
#include "problem.hpp"
#include "tape.hpp"

namespace sk {

#ifdef __HIP__
// A maximum that KEEPS a NaN (fmax drops it): a gradient entry that is not a number — a Jacobian entry that is not finite beside finite
// residuals — must reach the host, where the evaluation fails on it (evaluate_with_jacobian: isfinite of the gradient max-norm).
__device__ __forceinline__ double max_keep_nan(double a, double b) { return (b > a || b != b) ? b : a; }
#endif

void set_error(const char* fmt, ...);
const char* get_error();
void set_status(int status);  // status of the last failure that could only be reported as a null handle (sk_last_status)
int get_status();

#define SK_HIP_TRY(expr)                                                                 \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess) {                                                              \
      sk::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return SK_ERR_HIP;                                                                 \
    }                                                                                    \
  } while (0)

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  bool owned = true;
  DevBuf() {}
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p && owned) (void)hipFree(p);
    p = nullptr; n = 0; owned = true;
  }
  hipError_t alloc(size_t count) {
    release();
    n = count;
    if (count == 0) return hipSuccess;
    return hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T));
  }
  void adopt(T* ext, size_t count) { release(); p = ext; n = count; owned = false; }
  hipError_t upload(const std::vector<T>& h, hipStream_t s) {
    hipError_t e = alloc(h.size());
    if (e != hipSuccess || h.empty()) return e;
    return hipMemcpyAsync(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s);
  }
  hipError_t zero(hipStream_t s) { return n ? hipMemsetAsync(p, 0, n * sizeof(T), s) : hipSuccess; }
};

// A stream of a call's own, destroyed on every way out of it.
struct StreamGuard {
  hipStream_t s = nullptr;
  ~StreamGuard() { if (s) (void)hipStreamDestroy(s); }
};

// The loss nodes as a kernel takes them: a problem without any gets one trivial node, so that the pointer is never null.
inline std::vector<LossNode> loss_nodes_or_trivial(std::vector<LossNode> nodes) {
  if (nodes.empty()) { LossNode t; t.type = kLossTrivial; t.f = t.g = -1; t.depth = 0; t.a = t.b = 0.0; nodes.push_back(t); }
  return nodes;
}

struct Options {  // Solver.Options; Ceres 1.x defaults
  int linear_solver_type = SK_DENSE_QR;  // ceres default is SPARSE_NORMAL_CHOLESKY when built with a sparse backend, else DENSE_QR
  int linear_solver_type_given = -1;     // set when the solver in use is an alternate for the one asked for (capi.hip: make_solver)
  int minimizer_type = SK_TRUST_REGION;
  int trust_region_strategy_type = SK_LEVENBERG_MARQUARDT, dogleg_type = SK_TRADITIONAL_DOGLEG;
  int max_num_iterations = 50;
  bool progress_to_stdout = false;
  double function_tolerance = 1e-6, gradient_tolerance = 1e-10, parameter_tolerance = 1e-8;
  double initial_trust_region_radius = 1e4, max_trust_region_radius = 1e16, min_trust_region_radius = 1e-32;
  double min_relative_decrease = 1e-3, min_lm_diagonal = 1e-6, max_lm_diagonal = 1e32;
  bool jacobi_scaling = true;
  int max_num_consecutive_invalid_steps = 5;
  // CGNR (common.hpp: namespace cgnr): the preconditioner, the forcing sequence's eta, the bounds on the CG iterations of one linear solve
  int preconditioner_type = SK_JACOBI;
  double eta = 0.1;
  int max_linear_solver_iterations = 500, min_linear_solver_iterations = 0;
  bool cgnr_schur_elimination = false;  // sk_options_set_schur_elimination: CG on the implicit Schur complement of an independent set (cgnr_plan.hpp)
  // Inner iterations (common.hpp: namespace inner; inner_plan.hpp): off by default; the ordering's blocks with a group id each (empty: automatic)
  bool use_inner_iterations = false;
  double inner_iteration_tolerance = 1e-3;
  std::vector<double*> inner_ordering_blocks;
  std::vector<int> inner_ordering_groups;
  int device = -1;
  hipStream_t stream = nullptr;
  bool stream_set = false;
  int rank = 0, world = 1;
  sk_allreduce_fn allreduce = nullptr;
  void* allreduce_user = nullptr;
  int distribution_mode = SK_DISTRIBUTION_AUTO;
  void* reduce_buffer = nullptr;
  size_t reduce_buffer_bytes = 0;
  // SYRK depth in 128-column blocks (K = group * 128).  0 = automatic: 3 when the trailing SYRK is the long pole
  // (full factorisation; 2 and 4 within 1 %), 1 when the block envelope leaves so little of it that the serial
  // panel chain decides (measured on Ladybug-1723: 13.2 / 13.4 / 14.0 / 14.6 ms per iteration for 1 / 2 / 3 / 4).
  int cholesky_group = 0;
  int group_or(int automatic) const { return cholesky_group > 0 ? cholesky_group : automatic; }
  bool lookahead = true;   // potrf128 on a second stream, off the critical path
  int dissection = SK_DISSECTION_AUTO;  // DENSE_SCHUR: eliminate the head and the tail of a camera sequence side by side (sk_options_set_cholesky_dissection)
  bool envelope = true;    // DENSE_SCHUR: skip the blocks of the reduced system outside its block envelope (bit-identical result)
  bool resident_kernels = true;  // sk_options_set_resident_kernels: 0 = no kernel of this solver waits for another one (same plans, launch by launch)
  bool graph_replay = true;      // sk_options_set_graph_replay: launch-bound problems replay their iteration as a hipGraph
  int max_segments = 0;          // sk_options_set_max_segments: SEGMENTED / AUTO cut the camera sequence into at most this many segments (0: one per rank)
  int border = SK_BORDER_AUTO;  // DENSE_SCHUR: order the cameras of loop closures into a trailing border of the reduced system (sk_options_set_cholesky_border)
  int retained = SK_RETAINED_AUTO, retained_max = 0;  // DENSE_SCHUR: the points with the widest tracks stay in the reduced system (sk_options_set_retained_points)
};

// Traditional dogleg as published for Ceres 1.x's DoglegStrategy: recalled, not pinned (like SURVEY.md §8a row a13), so the
// constants live here and nowhere else.
namespace dogleg {
constexpr double kMinMu = 1e-8, kMaxMu = 1.0, kMuIncreaseFactor = 10.0;
constexpr double kIncreaseThreshold = 0.75, kDecreaseThreshold = 0.25;
constexpr double kRadiusDecreaseFactor = 0.5, kRadiusGrowth = 3.0, kMuDecrease = 2.0;  // mu <- max(min_mu, 2 mu / 10) after an accepted step
// the scalars of one linear solve: the observation products (w = J s, m = J g) and the vector norms in the diagonal-scaled space
struct Scalars {
  double w_r = 0, m_r = 0, w_w = 0, w_m = 0, m_m = 0, g_g = 0, g_p = 0, p_p = 0;
  static Scalars from(const double* k) { return {k[0], k[1], k[2], k[3], k[4], k[5], k[6], k[7]}; }  // in the order the kernels leave them
};
// step = a s + b g for this radius (s = -g_hat / diag, the Cauchy direction; g, the Gauss-Newton step), its norm in the
// diagonal-scaled space and the model's cost decrease.  false: no step can be formed from these scalars.
bool interpolate(const Scalars& k, double radius, double* a, double* b, double* step_norm, double* model_cost_change);
}  // namespace dogleg

// Parameter bounds: Ceres 1.x's constrained trust-region loop (projected steps with a backtracking Armijo line search), recalled,
// not pinned (like SURVEY.md §8a row a13), so the constants live here and nowhere else.  The interpolation is the one departure
// from Ceres' defaults: quadratic, from function values only (Ceres: CUBIC, which needs a Jacobian at every trial point).
namespace bounds {
constexpr double kSufficientDecrease = 1e-4;
constexpr double kMaxStepContraction = 1e-3, kMinStepContraction = 0.6;  // the next alpha lies inside [1e-3 alpha, 0.6 alpha]
constexpr int kMaxNumIterations = 20;                                     // contractions
constexpr double kMinStepSize = 1e-9;                                     // of alpha max_j |delta_j|
constexpr double kBisection = 0.5;                                        // after a trial whose cost is not finite
}  // namespace bounds

// CGNR: Ceres 1.x's ConjugateGradientsSolver on the damped normal equations, applied as two products with the block-sparse
// Jacobian; recalled, not pinned (like SURVEY.md §8a row a13), so the constants live here and nowhere else.
namespace cgnr {
constexpr int kResidualResetPeriod = 10;  // res = b - A x instead of res -= alpha q when it % 10 == 0
constexpr int kBatch = 8;                 // CG iterations enqueued between two reads of the done flag (SK_CGNR_BATCH)
constexpr int kPartSlots = 64;            // a column block's slot list is summed in parts of this many slots (cgnr_plan.hpp)
// how a linear solve ended ("cg_status_last" of sk_solver_stat); kRunning on the device only
enum Status { kConverged = 0, kIterationLimit = 1, kBreakdown = 2, kZeroRhs = 3, kRunning = -1 };
}  // namespace cgnr

// Inner iterations: Ceres 1.x's use_inner_iterations (block coordinate descent behind every trust-region step), recalled, not
// pinned (like SURVEY.md §8a row a13), so the constants live here and nowhere else.  One inner solve is the Levenberg-Marquardt
// loop of SolverBase::step on one parameter block with Ceres' DEFAULT options, whatever the outer solve's options are.
namespace inner {
constexpr int kMaxNumIterations = 50;
constexpr double kFunctionTolerance = 1e-6, kGradientTolerance = 1e-10, kParameterTolerance = 1e-8;
constexpr double kInitialRadius = 1e4, kMaxRadius = 1e16, kMinRadius = 1e-32;
constexpr double kMinRelativeDecrease = 1e-3, kMinLmDiagonal = 1e-6, kMaxLmDiagonal = 1e32;
constexpr int kMaxConsecutiveInvalidSteps = 5;
constexpr int kBatch = 4;  // rounds enqueued between two reads of the group's done flag (SK_INNER_BATCH)
// how a block's solve ended ("status" of sk_solver_inner_iteration_blocks); kRunning while it goes on
enum Status { kRunning = 0, kGradient = 1, kParameter = 2, kFunction = 3, kIterationLimit = 4, kInvalidSteps = 5, kRadius = 6 };
}  // namespace inner

struct IterationLog {
  int iteration = 0;
  double cost = 0, cost_change = 0, gradient_max_norm = 0, step_norm = 0, relative_decrease = 0,
         trust_region_radius = 0, iter_time = 0, total_time = 0;
  int step_is_valid = 1, step_is_successful = 1;
  double step_size = 1.0;           // the line search's alpha under parameter bounds
  int line_search_evaluations = 1;  // candidate costs evaluated in the iteration
  int linear_solver_iterations = 0; // CGNR: CG iterations of the iteration's linear solve (0 for the factorisation solvers)
  int inner_iteration_rounds = 0;   // use_inner_iterations: the lock-step rounds that refined this iteration's candidate
};

struct Summary {
  double initial_cost = 0, final_cost = 0;
  int num_successful_steps = 0, num_unsuccessful_steps = 0;
  int termination_type = SK_NO_CONVERGENCE;
  std::string message;
  std::vector<IterationLog> iterations;
  double phase_seconds[7] = {0, 0, 0, 0, 0, 0, 0};
  // problem / solver description for the reports
  int num_parameter_blocks = 0, num_parameters = 0, num_residual_blocks = 0;
  long num_residuals = 0;
  int linear_solver_type = 0;
  int linear_solver_type_given = -1;  // what Solver.Options asked for when the solver used is its alternate (Ceres: "Given / Used")
  int num_e_blocks = 0, num_f_blocks = 0;
  int world = 1;
  int trust_region_strategy_type = SK_LEVENBERG_MARQUARDT;
  int preconditioner_type = SK_JACOBI;  // CGNR
  long linear_solver_iterations = 0;    // CGNR: total over the solve
  bool schur_elimination = false;       // CGNR with sk_options_set_schur_elimination: the eliminated blocks and the columns CG runs on
  int eliminated_blocks = 0, reduced_columns = 0;
  bool use_inner_iterations = false;    // the report's inner-iterations lines appear with the option on alone
  int inner_iteration_groups = 0, inner_iteration_steps = 0;
  long inner_iteration_rounds = 0;
  bool inner_iterations_enabled = false;
  double inner_iteration_seconds = 0.0;
  std::string device_name;
  std::string brief, full;
  void build_reports();
};

// device copy of a tape (owned by a solver, or by one sk_cost_function_evaluate)
struct TapeDevBuffers {
  DevBuf<TapeIns> ins; DevBuf<double> consts; DevBuf<int32_t> out; DevBuf<int> param_block, param_index;
  TapeDev view;
  Tape host;
  hipError_t upload(const Tape& t, hipStream_t s);
};

const char* linear_solver_name(int t);
const char* termination_name(int t);

}  // namespace sk
