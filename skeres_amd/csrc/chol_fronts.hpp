// The fronts of sk_cholesky_solve*: a dense SPD system given by its lower triangle (row-major, n x n) and a right-hand side, laid
// out as the factorisation plans take it — one padded front, the head / tail / root of a two-way dissection, the R leaves and
// the root of a multi-way one — and the way back from the fronts' solutions to x.  Host index arithmetic alone, no device code in
// here: chol_solve.hip drives the device over these layouts, tools/chol_fronts_check.cpp carries the same steps out on the host.
#pragma once
#include <cstddef>
#include <string>
#include <vector>

#include "chol_envelope.hpp"

namespace sk {

// Block envelope of a front held on the host (lower triangle, row-major, ld): first non-zero block column per block row.
std::vector<int> host_block_first_cols(const std::vector<double>& M, size_t ld, int nblk);
std::vector<int> host_block_envelope(const std::vector<double>& M, size_t ld, int nblk, int tail_rows = 1);

// A front on the host: dim = nblk * 128 rows, of which the first ncols block columns are factored (a root: all of them).
struct HostFront {
  size_t dim = 0;
  int nblk = 0, ncols = 0, rhs_row = 0;
  std::vector<double> F;    // dim x dim, lower triangle
  std::vector<int> last;    // block envelope (empty: none)
};

// --- one front: the system, the right-hand side as row n (1e300 on its diagonal), identity on the padding ---
struct SingleFront {
  int n = 0, npad = 0, nblk = 0, rhs_row = 0;
  std::vector<double> S;
  std::vector<int> last, tail;  // the bordered envelope of the matrix itself (border_begin_row >= 0); empty otherwise
};
inline int single_front_blocks(int n) { return (n + 1 + 127) / 128; }
// a caller's envelope (single_front_blocks(n) entries): the first block column at which it is not one, -1 if it is
int invalid_envelope_column(int n, const int* last);
// border_begin_row >= 0: rows from there on are the border (cholesky_envelope_bordered)
SingleFront single_front(int n, const double* A, const double* b, int border_begin_row);
void single_front_solution(const SingleFront& f, const std::vector<double>& y, double* x);  // y: the front's solution (npad)
void single_front_factor(const SingleFront& f, const std::vector<double>& S, double* L);    // L (n x n, tril) out of the factored front

// --- two-way dissection: head [0, head), separator [head, tail_begin), tail [tail_begin, n) in REVERSE order ---
struct TwoWayFronts {
  int n = 0, head = 0, tail_n = 0, sep_n = 0, border_blocks = 0;
  HostFront A, B, R;        // head, tail, root
  std::vector<int> mapB;    // the tail's border index -> root index (< 0: padding)
};
// empty: the tail does not couple with the head; otherwise the message that says where it does
std::string two_way_check(int n, const double* A, int head, int tail_begin);
TwoWayFronts two_way_fronts(int n, const double* A, const double* b, int head, int tail_begin);
void two_way_scatter(const TwoWayFronts& f, const double* y, double* x);  // y = yA | yB | yR, each of its front's dim

// --- multi-way dissection: R segments with R - 1 separators between them ---
// separator k (1 <= k < R) = rows [sb[k], se[k]); segment k = rows [se[k], sb[k + 1]) with se[0] = 0, sb[R] = n
struct SegmentCuts {
  int R = 0, n = 0, nroot = 0;
  std::vector<int> sb, se;
  std::vector<int> sep_off;  // sep_off[k - 1]: offset of separator k in the root; sep_off[R - 1]: total (nroot)
  int root_index(int row) const;  // global row of a separator -> root index (-1: not a separator's)
};
// empty: cuts (2 (R - 1) entries: begin, end of each separator) are valid and separate A; otherwise the message
std::string segment_cuts(int n, const double* A, int R, const int* cuts, SegmentCuts* out);
HostFront segments_root(const SegmentCuts& c, const double* A, const double* b);  // every separator in order, then the right-hand side
struct LeafFront {
  SegmentLayout L;
  size_t dim = 0;
  int interior_n = 0;
  std::vector<int> order;   // front row -> global row (-1: padding / right-hand side)
  std::vector<int> map;     // border index -> root index (the right-hand side's: nroot; < 0: padding)
  std::vector<int> gmap;    // ... for the gather of the border's unknowns: the right-hand side's row is none (-1)
  std::vector<int> last;
  std::vector<double> F;    // may be released once it is on the device
};
LeafFront segment_leaf(const SegmentCuts& c, const double* A, const double* b, int k);
void segments_scatter_root(const SegmentCuts& c, const double* yR, double* x);
void segments_scatter_leaf(const LeafFront& f, const double* y, double* x);

}  // namespace sk
