// The host mirror of the reference's Problem and the plain types it is made of — plain C++: the host planning of the
// reduced system (bal_plan.cpp) reads a Problem and is compiled without the device headers.  The device side of each type
// lives where it did: loss.hpp, parameterization.hpp, tape.hpp (which include this file).
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/skeres_amd.h"

namespace sk {

// ---- loss.hpp ----
enum LossType : int {
  kLossTrivial = 0, kLossHuber = 1, kLossSoftLOne = 2, kLossCauchy = 3, kLossTukey = 4, kLossTolerant = 5, kLossComposed = 6, kLossScaled = 7
};

// One node of a flattened loss expression: children come before their parent.
struct LossNode {
  int type;
  int f, g;     // children (composed: rho = f(g(s)); scaled: f), -1 = none (scaled: the NULL loss, rho = a s)
  int depth;    // nesting depth below this node (leaves: 0)
  double a, b;
};

// ---- parameterization.hpp ----
enum ParameterizationType : int { kParamIdentity = 0, kParamSubset = 1, kParamQuaternion = 2, kParamHomogeneousVector = 3, kParamConstant = 4 };

// ---- tape.hpp ----
struct TapeIns { int32_t op, dst, a, b, c; };  // dst: register; a, b, c: operands (SELECT: a = condition, b = then, c = else)

// host copy (owned by the cost function, interned per problem by content)
struct Tape {
  int num_residuals = 0, num_registers = 0, num_obs_consts = 0;
  std::vector<int> block_sizes;
  std::vector<TapeIns> ins;
  std::vector<double> consts;
  std::vector<int32_t> out;  // operand per residual
  int dim() const { int d = 0; for (int b : block_sizes) d += b; return d; }
  std::string key() const;   // content key
};
constexpr int kTapeFunctorBase = 1000;  // Problem::rb_functor of a tape block = kTapeFunctorBase + index into Problem::tapes
// derivative slots per pass of the DENSE_SCHUR evaluation kernels' interpreter (defined beside them); 0: the tape's register file does not fit the LDS
int bal_tape_width(const Tape& t);

// ---- host mirror of the reference objects ----------------------------------
struct CostFunction {  // com.google.ceres.CostFunction as sized by CORE/SizedCostFunction.scala
  int functor_id = 0;
  std::vector<double> consts;
  sk_evaluate_fn callback = nullptr;
  void* user = nullptr;
  int num_residuals = 0;
  std::vector<int> block_sizes;
  std::shared_ptr<const Tape> tape;  // SK_FUNCTOR_TAPE: the recorded body (consts: the captured doubles of THIS cost function)
};

// PredefinedLossFunctions (ceres.i:159-184): a flattened expression, children before parents; empty == trivial
struct LossFunction {
  std::vector<LossNode> nodes;
  int root() const { return nodes.empty() ? -1 : (int)nodes.size() - 1; }
};

// PredefinedLocalParameterizations (ceres.i:186-210)
struct LocalParameterization {
  int type = kParamIdentity, global_size = 0, local_size = 0;
  unsigned constant_mask = 0;  // subset: bit i = coordinate i held constant
};

struct Problem {  // CeresProblem; parameter blocks identified by pointer value
  std::unordered_map<double*, int> block_of;
  std::vector<double*> block_ptr;
  std::vector<int> block_size;
  // residual blocks (compact form)
  std::vector<int> rb_functor;
  std::vector<int> rb_num_residuals;
  std::vector<size_t> rb_const_off;
  std::vector<size_t> rb_pidx_off;  // size = blocks + 1
  std::vector<int> rb_pidx;
  std::vector<double> consts;
  std::vector<const CostFunction*> rb_cost;  // non-null only for host-callback blocks
  // recorded functor bodies, every distinct one once (by content: the caller may free its cost function); a tape block's
  // rb_functor is kTapeFunctorBase + its index here
  std::vector<std::shared_ptr<const Tape>> tapes;
  std::unordered_map<std::string, int> tape_of;
  int intern_tape(const std::shared_ptr<const Tape>& t) {
    const std::string k = t->key();
    auto it = tape_of.find(k);
    if (it != tape_of.end()) return it->second;
    tapes.push_back(t);
    tape_of.emplace(k, (int)tapes.size() - 1);
    return (int)tapes.size() - 1;
  }
  const Tape* tape_of_block(size_t b) const { const int f = rb_functor[b]; return f >= kTapeFunctorBase ? tapes[f - kTapeFunctorBase].get() : nullptr; }
  // loss functions: every distinct loss expression once in loss_nodes (copied: the caller may free its object);
  // rb_loss[b] = root node of block b's loss, -1 = trivial
  std::vector<LossNode> loss_nodes;
  std::vector<int> rb_loss;
  std::unordered_map<std::string, int> loss_root_of;
  bool has_loss = false;
  int intern_loss(const LossFunction* l);
  // local parameterizations: block_param[b] = index into params (copied: the caller may free its object), -1 = none;
  // block_constant[b]: Problem::SetParameterBlockConstant
  std::vector<LocalParameterization> params;
  std::vector<int> block_param;
  std::vector<char> block_constant;
  bool has_parameterization() const {
    for (size_t b = 0; b < block_ptr.size(); ++b)
      if ((b < block_param.size() && block_param[b] >= 0) || (b < block_constant.size() && block_constant[b])) return true;
    return false;
  }
  // Problem::SetParameterLowerBound / SetParameterUpperBound (ceres/problem.h via ceres.i:150): per block, allocated when a bound
  // is first set (block_size entries, -/+ infinity where nothing is set); a problem without bounds carries two empty vectors
  std::vector<std::vector<double>> block_lower, block_upper;
  double lower_bound(size_t b, int i) const { return b < block_lower.size() && !block_lower[b].empty() ? block_lower[b][i] : -std::numeric_limits<double>::infinity(); }
  double upper_bound(size_t b, int i) const { return b < block_upper.size() && !block_upper[b].empty() ? block_upper[b][i] : std::numeric_limits<double>::infinity(); }
  void set_bound(size_t b, int i, double v, bool upper) {
    std::vector<std::vector<double>>& t = upper ? block_upper : block_lower;
    if (t.size() <= b) { if (std::isinf(v)) return; t.resize(block_ptr.size()); }
    if (t[b].empty()) { if (std::isinf(v)) return; t[b].assign(block_size[b], upper ? std::numeric_limits<double>::infinity() : -std::numeric_limits<double>::infinity()); }
    t[b][i] = v;
  }
  bool block_has_bounds(size_t b) const {
    for (int i = 0; i < block_size[b]; ++i) if (std::isfinite(lower_bound(b, i)) || std::isfinite(upper_bound(b, i))) return true;
    return false;
  }
  bool has_bounds() const {  // some coordinate has a finite bound
    if (block_lower.empty() && block_upper.empty()) return false;
    for (size_t b = 0; b < block_ptr.size(); ++b) if (block_has_bounds(b)) return true;
    return false;
  }
  long num_residuals = 0;
  bool has_callbacks = false;
  Problem() { rb_pidx_off.push_back(0); }
  int num_parameters() const { long s = 0; for (int b : block_size) s += b; return (int)s; }
};

}  // namespace sk
