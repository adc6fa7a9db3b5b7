// What the users of Problem::Evaluate's block-sparse Jacobian share on the host (cgnr_plan.hpp, covariance_plan.hpp): the tangent
// columns of the parameter blocks that move, the cutting of a summation list into parts, the independent set that a Schur
// elimination removes, and the refusal of blocks that are too
// large for one lane — plain C++ over a Problem and an EvaluatePlan, compiled without the device headers like evaluate_plan.cpp.
#pragma once
#include <string>
#include <vector>

#include "evaluate_plan.hpp"

namespace sk {

constexpr int kCgnrPartSlots = 64;  // == cgnr::kPartSlots (common.hpp; static_assert in cgnr_solver.hip)

// Columns.  The tangent vector holds the parameter blocks that move, in problem order, each with its tangent size; a constant
// block and a block whose tangent size is 0 have no columns (Problem::Evaluate keeps a constant block's columns; its values array
// has no entries for them either way, so the values layout is shared).
struct TangentColumns {
  int num_cols = 0, num_ambient = 0;  // tangent size of the problem, size of x
  std::vector<int> block_off;         // [parameter blocks + 1] in x
  // per parameter block: ParameterizationType (kParamConstant for constant blocks), size, tangent size (of a constant block: see
  // ConstantTangent) and first column (-1: constant, or tangent size 0)
  std::vector<int> pb_type, pb_size, pb_local_size, pb_local_off;
  std::vector<unsigned> pb_mask;
  std::vector<int> cb_col, cb_size, cb_block;  // column blocks (the parameter blocks that move): first column, tangent size, parameter block
  std::vector<int> cb_of;                      // per parameter block: its column block (-1: none)
};
// The one rule the users differ in: the tangent size that pb_local_size reports for a constant block.
enum class ConstantTangent {
  kZero,  // 0, as the solvers count it (CGNR)
  kKeep   // Problem::Evaluate's, so that a covariance block of a constant parameter block keeps its shape (Covariance)
};
void tangent_columns_build(const Problem& p, const EvaluatePlan& E, ConstantTangent constants, TangentColumns* columns);

// Parts.  Owner q sums the entries [begin_of[q], begin_of[q + 1]) of some list.  The range is cut into PARTS of kCgnrPartSlots
// entries, the last one shorter; an empty range still has one empty part.  An owner of more than one part (a LONG owner) leaves
// one partial sum per part, which a second launch adds in part order: out numbers them consecutively.
struct PartList {
  std::vector<int> owner, begin, end;   // per part: its owner and its range of the list
  std::vector<int> out;                 // -1: the owner's only part; else the index of its partial sum
  std::vector<int> long_owner, long_begin;  // long owners; [long owners + 1] their ranges of partial sums
  int num_partials = 0;
};
void cut_parts(const std::vector<int>& begin_of, PartList* parts);

// The independent set of a Schur elimination (covariance_plan.hpp, cgnr_plan.hpp).  Two column blocks are neighbours when a residual
// block names both; nb[nb_begin[c] .. nb_begin[c + 1]) are the DISTINCT neighbours of column block c.  The blocks are visited in
// ascending order of (number of distinct neighbours, column block), which ascends with the parameter-block index, and a block
// joins the set when none of its neighbours is in it.  in_set: per column block 1 or 0.
void greedy_independent_set(const std::vector<int>& nb_begin, const std::vector<int>& nb, std::vector<int>* in_set);

// "" when every parameter block fits one lane, else why not, in `feature`'s name ("CGNR", "Covariance"): a parameterized block of
// size above `limit`, or a tangent size above it.  constants_too: constant blocks are held to the limit as well.
std::string block_size_refusal(const Problem& p, const char* feature, int limit, bool constants_too);

}  // namespace sk
