// Host plan of sk_covariance_compute (covariance.hip): the block-sparse Jacobian's layout is Problem::Evaluate's (evaluate_plan.hpp)
// over every residual block and every parameter block, the columns are jacobian_plan.hpp's TangentColumns (the parameter blocks that
// move, in problem order, each with its tangent size); this plan adds what the normal matrix H = J^T J and the selection of the requested
// covariance blocks need — plain C++ over a Problem, compiled without the device headers like cgnr_plan.cpp.
//
// Normal-matrix pairs.  For every unordered pair of column blocks (i >= j by first column, i == j included) that share a
// residual block, the TERMS of H_ij = sum J_i^T J_j: (slot of i, slot of j) of every residual block that stores both, in row order.
// A term list is cut into PARTS of cgnr::kPartSlots (64) terms (jacobian_plan.hpp: cut_parts); a pair of more than one part (a LONG pair:
// a camera's diagonal, a hub of a chain) leaves one partial tile per part, which a second launch adds in part order.  Pairs, terms
// and parts are fixed here: the sum of a tile depends on the problem alone, and no launch uses a floating-point atomic.
//
// Selection.  The distinct moving column blocks named by the requested pairs, in order of first appearance; their k columns are
// the unit rows of the border behind H, and every requested pair knows where its block sits in the k x k result.
//
// Schur elimination (sk_covariance_options_set_schur_elimination; off by default, and then nothing below exists in the plan).
// The eliminated set E is a greedy independent set over the moving column blocks, two of which are NEIGHBOURS when a residual
// block stores both: the blocks are visited in ascending order of (number of distinct neighbours, parameter-block index), and a
// block joins E when none of its neighbours is in E yet; F is the rest, in problem order.  (Bundle adjustment: the points, and
// every camera stays in F because it neighbours a point of low degree; a chain: alternating blocks, the hub in F; a block that no
// residual block names has degree 0 and joins E first.)  E depends on the problem alone.  With H = [[U, W], [W^T, V]], V block
// diagonal over E, the pairs, terms and parts above stay as they are and are ROUTED: an (e, e) or (f, e) pair sums into a TILE of
// kCovarianceTile doubles (tile t < |E|: V_e of the t-th e-block, later L_e; tile |E| + t: L_e^-1; then one tile per (f, e) pair,
// rows of f by columns of e whichever of the two has the lower column), an (f, f') pair into the dense matrix, now n_F wide.
// SCHUR TERMS: for every pair of F blocks (g >= g' by first column, g == g' included) that share an e-block, (tile of (g, e), tile
// of (g', e)) per shared e in ascending order of e, cut into parts of 64 with the same long-pair mechanism.  A (g, e) tile is the
// sum over all residual blocks on that pair.  F(e): the F-neighbours of e in ascending column order.  The selection is the requested
// F blocks and, for every requested e, all of F(e); sel_col holds columns of the reduced matrix.
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
  TangentColumns cols;  // num_cols is N; a constant block keeps Problem::Evaluate's tangent size (its covariance block is zero, of that shape)
  // the normal matrix
  std::vector<int> pair_i, pair_j;      // column blocks, first column of i >= first column of j
  std::vector<int> pair_begin;          // [pairs + 1] into term_si / term_sj
  std::vector<int> term_si, term_sj;    // slots of eval, both of one residual block
  PartList pair_parts;                  // of the term lists, in pair order; a partial sum is a tile
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
  // Schur elimination (empty / 0 unless the plan was built with it)
  bool schur = false;
  std::vector<int> cb_elim;   // per column block: 1 in E, 0 in F
  std::vector<int> cb_red;    // per column block: in F its first column of the reduced matrix, in E its index among the e-blocks
  int num_elim = 0, red_cols = 0, num_tiles = 0;
  long long schur_terms = 0;
  std::vector<int> pair_tile, pair_flip;      // per pair: its tile (-1: the dense matrix); 1: the pair's i is the e-block, the tile is stored transposed
  std::vector<int> e_cb;                      // the e-blocks (column blocks), ascending
  std::vector<int> ew_begin;                  // [e-blocks + 1] F(e) as ranges of the three lists below
  std::vector<int> ew_tile, ew_g, ew_sel;     // the (g, e) tile, the F column block g, g's first row among the k selected ones (-1: e was not requested)
  std::vector<int> sp_i, sp_j, sp_begin;      // pairs of F blocks with Schur terms; [pairs + 1] into st_*
  std::vector<int> st_a, st_b, st_ne;         // tile of (g, e), tile of (g', e), tangent size of e
  PartList schur_parts;                       // of the Schur terms, in sp_* order
  std::vector<int> req_ea, req_eb;            // per requested pair: the e-block index of a / b (-1: in F, req_ra / req_rb hold its rows)
};

// "" when the covariance of this problem can be computed, else why not (SK_ERR_UNSUPPORTED): dense rows, a tangent size (or the
// size of a parameterized block) above kCovarianceMaxBlock, more than kCovarianceMaxColumns columns (schur: not checked here — the
// plan counts the columns that are left after the elimination).  Host data alone.
std::string covariance_refusal(const Problem& p, bool schur = false);
// pairs: parameter blocks of the problem (indices), as requested.  Returns an sk_status; *why says what is wrong.  schur: with the
// elimination (SK_ERR_UNSUPPORTED for more than kCovarianceMaxColumns reduced columns or more than INT_MAX Schur terms).
int covariance_plan_build(const Problem& p, const std::vector<std::pair<int, int>>& pairs, CovariancePlan* plan, std::string* why, bool schur = false);

}  // namespace sk
