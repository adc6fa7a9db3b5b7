// ceres::Covariance on the device (covariance.hip): blocks of (J^T J)^-1 by the normal-equations Cholesky.  Plan:
// covariance_plan.hpp; kernels: covariance_kernels.hip; the factorisation: cholesky_factor (chol_kernels.hip).
#pragma once
#include <map>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "common.hpp"

namespace sk {

struct CovarianceOptions {  // ceres::Covariance::Options (algorithm_type, null_space_rank, num_threads: no counterpart)
  bool apply_loss_function = true;
  double min_reciprocal_condition_number = 1e-14;
  int device = -1;  // -1: the current device
  bool schur_elimination = false;  // (no reference counterpart) eliminate an independent set of blocks in front of the factorisation: covariance_plan.hpp
};

constexpr int kCovariancePhases = 5;  // 0 evaluation, 1 assembly and scaling, 2 factorisation, 3 extraction, 4 downloads

class Covariance {
 public:
  explicit Covariance(const CovarianceOptions& o) : opt_(o) {}
  // pairs (blocks1[i], blocks2[i]); an sk_status
  int compute(const Problem& p, double* const* blocks1, double* const* blocks2, int num_pairs);
  int get_block(const double* b1, const double* b2, bool tangent, double* out) const;
  int get_matrix(double* const* blocks, int n, bool tangent, double* out) const;
  int stat(const char* name, double* value) const;
  int block_sizes(const double* block, int* size, int* tangent_size) const;

 private:
  int run(const Problem& p, const std::vector<std::pair<int, int>>& pairs);
  CovarianceOptions opt_;
  bool valid_ = false, has_stats_ = false;
  // what the getters serve: host memory, laid out by the plan of the last successful compute
  std::unordered_map<const double*, int> block_of_;
  std::vector<int> size_, tangent_;
  std::map<std::pair<int, int>, int> req_of_;
  std::vector<long> tan_off_, amb_off_;
  std::vector<double> out_;
  std::map<std::string, double> stats_;
};

// Steps 3 to 6 of a compute on a matrix given as such (the testing library's entry, tests/test_gpu_covariance.py "border route"):
// H (n x n, row-major, symmetric positive definite; its lower triangle is read) is scaled, bordered with the columns of the selected
// blocks — consecutive blocks of `block` columns, the last one shorter —, factored, and the selected k x k block of its inverse
// extracted into out (row-major, the blocks in the order given).  *ratio: min L_jj^2 / max L_jj^2 of the scaled matrix's factor.
int covariance_border_route(int n, const double* H, int block, const int* sel_blocks, int num_sel, double* out, double* ratio);

}  // namespace sk
