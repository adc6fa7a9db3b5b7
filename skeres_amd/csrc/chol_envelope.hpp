// The block envelope of a symmetric matrix of 128-blocks and the host arithmetic on it: which block rows a block column
// reaches, the flops and the groups of a factorisation inside it, the layouts of the fronts of a dissected system.
// No device code in here: the host planning (bal_plan.cpp) and the host side of the Cholesky kernels share it.
#pragma once
#include <algorithm>
#include <vector>

namespace sk {

// A block envelope as cholesky_factor takes it, by reference (the arrays are the caller's): block column c of the factor is
// non-zero in a contiguous run of block rows down to last[c] (among rows 0 .. nblk - 2; nullptr: every row), and in the TAIL rows
// [tail[c], nblk) on top of it (nullptr: the uniform last tail_rows block rows; the final block row carries the right-hand side
// and is active everywhere).  ncols < nblk: a partial factorisation — only the first ncols block columns are factored (a leaf
// front; only such a front has more than one uniform tail row).  The clamps every reader applied are applied once, here.
struct BlockEnvelope {
  int nblk, ncols, tail_rows;
  const int* last;
  const int* tail;
  BlockEnvelope(int nblk_, const int* last_, const int* tail_ = nullptr, int ncols_ = -1, int tail_rows_ = 1)
      : nblk(nblk_), ncols(ncols_ < 0 || ncols_ > nblk_ ? nblk_ : ncols_), tail_rows(tail_rows_), last(last_), tail(tail_) {
    if (tail_rows < 1 || ncols > nblk - tail_rows) tail_rows = 1;
  }
  int last_row(int col) const { return last && last[col] < nblk - 1 ? last[col] : nblk - 1; }  // end of the column's run
  int tail_begin(int col) const { return tail ? tail[col] : nblk - tail_rows; }                // first tail row the column reaches
  // active block rows of block column col from block row first_row on: what is left of its run, and the tail rows behind it
  int active_rows(int col, int first_row) const {
    const int lr = last_row(col);
    const int main_rows = lr >= first_row ? lr - first_row + 1 : 0;
    return main_rows + std::max(0, nblk - std::max(tail_begin(col), first_row + main_rows));
  }
  int height(int col) const { return active_rows(col, col + 1); }  // ... below the diagonal block
  double blocks() const { double in = 0.0; for (int c = 0; c < ncols; ++c) in += active_rows(c, c); return in; }  // 128-blocks that are factored or updated
};

// The groups of block columns a factorisation runs in (defined beside the Cholesky kernels: they depend on their tuning constants).
struct CholeskyPlan {
  std::vector<int> bounds;  // group start columns + nblk
  std::vector<char> resident;  // per block column: under the resident panel chain
  std::vector<char> paired;    // ... as the first (1) / second (2) column of a resident pair (one K = 256 SYRK for both); else 0
};
CholeskyPlan cholesky_plan(int nblk, int group, const int* last, bool chain, int ncols = -1, int tail_rows = 1, const int* tail = nullptr);
int cholesky_plan_max_group(const CholeskyPlan& plan);
// --- multi-way dissection: R segments of a block-banded system with R - 1 separators between them ---
// Leaf front of one segment, in scalar rows.  The interior is followed by a border:
//   first segment    [right separator, forward | rhs]                         tail_rows 1 — the head of the two-way case
//   last segment     [left separator, REVERSED | rhs], interior reversed too  tail_rows 1 — the tail of the two-way case
//   between two      [right separator, forward, padded to whole blocks | left separator, forward | rhs]
//                    eliminated front to back: its last columns reach the right separator as part of their contiguous run;
//                    the left separator couples with the FIRST columns and fills in along the whole interior (the spike):
//                    its block rows are the tail rows of the partial factorisation (cholesky_plan).
struct SegmentLayout {
  int ncols = 0, nblk = 0, tail_rows = 1;
  int rhs_row = 0;                    // absolute row of the right-hand side in the front
  int right_off = -1, left_off = -1;  // first border row (relative to the border) of the right / left separator; -1: none
  bool reversed = false;
  bool spike = false;                 // a segment between two separators: the left one's rows reach every interior column
};
inline SegmentLayout segment_layout(int interior_n, int left_n, int right_n) {
  SegmentLayout L;
  L.ncols = (interior_n + 127) / 128;
  if (left_n <= 0) {          // first segment (or the only one)
    L.right_off = 0;
    L.nblk = L.ncols + (right_n + 1 + 127) / 128;
    L.rhs_row = L.ncols * 128 + right_n;
  } else if (right_n <= 0) {  // last segment
    L.left_off = 0; L.reversed = true;
    L.nblk = L.ncols + (left_n + 1 + 127) / 128;
    L.rhs_row = L.ncols * 128 + left_n;
  } else {
    const int rb = (right_n + 127) / 128;
    L.right_off = 0; L.left_off = rb * 128; L.spike = true;
    L.tail_rows = (left_n + 1 + 127) / 128;
    L.nblk = L.ncols + rb + L.tail_rows;
    L.rhs_row = L.ncols * 128 + L.left_off + left_n;
  }
  return L;
}
// Block envelope of the root (every separator in sequence order, then the right-hand side): separator k couples with
// separator k - 1 through the Schur complement of the segment between them.  sep_off: R entries, scalar offset of each
// separator in the root and, last, their total.  Empty result: dense (one separator).
// members_n > 0: that many scalar rows behind the last separator couple with EVERY separator (the members of a border: pseudo-cameras of
// retained points) — a border of the root in the sense of cholesky_envelope_bordered, its profile in *tail_out.
std::vector<int> root_envelope(const std::vector<int>& sep_off, int members_n = 0, std::vector<int>* tail_out = nullptr);

double cholesky_syrk_flops(int npad, int group, const int* last = nullptr, bool chain = false, double* c_tiles = nullptr, int ncols = -1, int tail_rows = 1,
                           const int* tail = nullptr);
double cholesky_plan_flops(int nblk, const int* last, int ncols = -1, int tail_rows = 1, const int* tail = nullptr);
std::vector<int> cholesky_envelope_last(const std::vector<int>& first_col, int tail_rows = 1);
// Bordered envelope of a whole system: block rows [border_begin, nblk) are the border (the last one carries the right-hand side).
// From the block rows' first non-zero block columns: last[c] over the rows before the border (nblk - 1 for the border's own
// columns), and the profile tail[c] = first border row active in column c — a border row, once reached, stays active, and so
// does every border row behind it (the caller orders the border so that the rows reached first come last).
void cholesky_envelope_bordered(const std::vector<int>& first_col, int border_begin, std::vector<int>* last, std::vector<int>* tail);
// first block column in which block row i is active, for every i (from the envelope: the run `last`, the tail profile or uniform tail)
std::vector<int> cholesky_row_first_cols(int nblk, const int* last, const int* tail, int tail_rows = 1);
std::vector<int> cholesky_group_bounds(int nblk, int group);

}  // namespace sk
