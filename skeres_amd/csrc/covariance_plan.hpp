// Host plan of sk_covariance_compute (covariance.hip): the block-sparse Jacobian's layout is Problem::Evaluate's (evaluate_plan.hpp)
// over every residual block and every parameter block, the columns are CGNR's (cgnr_plan.hpp: the parameter blocks that move, in
// problem order, each with its tangent size); this plan adds what the normal matrix H = J^T J and the selection of the requested
// covariance blocks need — plain C++ over a Problem, compiled without the device headers like cgnr_plan.cpp.
//
// Normal-matrix pairs.  For every unordered pair of column blocks (i >= j by first column, i == j included) that share a
// residual block, the TERMS of H_ij = sum J_i^T J_j: (slot of i, slot of j) of every residual block that stores both, in row order.
// A term list is cut into PARTS of cgnr::kPartSlots (64) terms, the last one shorter; a pair of more than one part (a LONG pair: a
// camera's diagonal, a hub of a chain) leaves one partial tile per part, which a second launch adds in part order.  Pairs, terms
// and parts are fixed here: the sum of a tile depends on the problem alone, and no launch uses a floating-point atomic.
//
// Selection.  The distinct moving column blocks named by the requested pairs, in order of first appearance; their k columns are
// the unit rows of the border behind H, and every requested pair knows where its block sits in the k x k result.
#pragma once
#include <string>
#include <utility>
#include <vector>

#include "cgnr_plan.hpp"
#include "evaluate_plan.hpp"

namespace sk {

// (N + k padded to blocks of 128)^2 doubles is the memory of one compute: a cap on memory, not a measurement
constexpr int kCovarianceMaxColumns = 32768;
constexpr int kCovarianceMaxBlock = kCgnrMaxBlock;  // tangent size (and size of a parameterized block), as CGNR
constexpr int kCovarianceTile = 256;                // entries of a partial tile: (at most 16) x (at most 16)

struct CovariancePlan {
  EvaluatePlan eval;  // staging sized for residuals + Jacobian planes
  int num_cols = 0;   // N: the tangent size of the problem
  std::vector<int> block_off;                                       // [parameter blocks + 1] in x
  std::vector<int> pb_type, pb_size, pb_local_size, pb_local_off;   // per parameter block: ParameterizationType (kParamConstant for constant blocks), size, tangent
                                                                    // size (Problem::Evaluate's, kept for a constant block) and first column (-1: constant, or tangent size 0)
  std::vector<unsigned> pb_mask;
  std::vector<int> cb_col, cb_size, cb_block;  // column blocks (the parameter blocks that move): first column, tangent size, parameter block
  // the normal matrix
  std::vector<int> pair_i, pair_j;      // column blocks, first column of i >= first column of j
  std::vector<int> pair_begin;          // [pairs + 1] into term_si / term_sj
  std::vector<int> term_si, term_sj;    // slots of eval, both of one residual block
  std::vector<int> part_pair, part_begin, part_end;  // the pair; the part's range of terms
  std::vector<int> part_out;                         // -1: the pair's only part; else the index of its partial tile
  std::vector<int> long_pair, long_begin;            // long pairs; [long pairs + 1] their ranges of partial tiles
  int num_partials = 0;
  // the selection
  std::vector<int> sel_cb;   // selected column blocks, in order of first appearance
  std::vector<int> sel_off;  // [selected + 1] first of the block's columns among the k selected ones
  std::vector<int> sel_col;  // [k] the column of H
  int k = 0;
  // the requested pairs, each once, (a, b) with parameter block a <= b; duplicates and the swapped order map to the same entry
  std::vector<int> req_a, req_b;
  std::vector<int> req_ra, req_rb;            // first row / column inside the k x k result (-1: a constant block, the covariance is zero)
  std::vector<long> req_tan_off, req_amb_off; // first entry of the tangent (tangent(a) x tangent(b)) and ambient (size(a) x size(b)) block in the packed output
  long out_size = 0;
};

// "" when the covariance of this problem can be computed, else why not (SK_ERR_UNSUPPORTED): dense rows, a tangent size (or the
// size of a parameterized block) above kCovarianceMaxBlock, more than kCovarianceMaxColumns columns.  Host data alone.
std::string covariance_refusal(const Problem& p);
// pairs: parameter blocks of the problem (indices), as requested.  Returns an sk_status; *why says what is wrong.
int covariance_plan_build(const Problem& p, const std::vector<std::pair<int, int>>& pairs, CovariancePlan* plan, std::string* why);

}  // namespace sk
