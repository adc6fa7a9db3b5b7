// Host arithmetic on block envelopes (chol_envelope.hpp).
#include "chol_envelope.hpp"

namespace sk {

// Algorithmic flops of factoring the blocks inside the envelope (last == nullptr: every block): per block column with
// h active block rows below it, 128^3 (1/3 + h + h^2) — diagonal factorisation, triangular solve of h blocks, symmetric
// update of h (h + 1) / 2 blocks with its diagonal blocks counted once.  Sums to n^3 / 3 for a full matrix.
double cholesky_plan_flops(int nblk, const int* last, int ncols, int tail_rows, const int* tail) {
  double f = 0.0;
  const BlockEnvelope env(nblk, last, tail, ncols, tail_rows);
  for (int c = 0; c < env.ncols; ++c) {
    const double h = env.height(c);
    f += 128.0 * 128.0 * 128.0 * (1.0 / 3.0 + h + h * h);
  }
  return f;
}

std::vector<int> root_envelope(const std::vector<int>& sep_off, int members_n, std::vector<int>* tail_out) {
  const int nsep = (int)sep_off.size() - 1;
  if (nsep <= 1) return {};
  const int total = sep_off[nsep] + (members_n > 0 ? members_n : 0), nblk = (total + 1 + 127) / 128;
  std::vector<int> first_col(nblk);
  for (int i = 0; i < nblk; ++i) first_col[i] = i;
  for (int k = 0; k < nsep; ++k) {
    const int col = sep_off[k > 0 ? k - 1 : 0] / 128;
    for (int r = sep_off[k] / 128; r <= (sep_off[k + 1] - 1) / 128 && r < nblk; ++r) first_col[r] = std::min(first_col[r], col);
  }
  if (members_n > 0 && tail_out) {
    const int border_begin = sep_off[nsep] / 128;
    for (int r = border_begin; r < nblk; ++r) first_col[r] = 0;
    std::vector<int> last;
    cholesky_envelope_bordered(first_col, border_begin, &last, tail_out);
    return last;
  }
  return cholesky_envelope_last(first_col);
}

// Envelope from the block rows' first non-zero block columns (first_col[i] <= i for i < nblk-1; the entry of the
// last block row is ignored: that row is always active): last[c] = max{ i <= nblk-2 : first_col[i] <= c }.
std::vector<int> cholesky_envelope_last(const std::vector<int>& first_col, int tail_rows) {
  const int nblk = (int)first_col.size();
  if (tail_rows < 1) tail_rows = 1;
  std::vector<int> last(nblk);
  for (int c = 0; c < nblk; ++c) last[c] = c < nblk - 1 ? c : nblk - 1;
  for (int i = 0; i + tail_rows < nblk; ++i) { const int c = first_col[i] < i ? first_col[i] : i; if (c >= 0 && last[c] < i) last[c] = i; }  // (the tail rows are active in every column anyway)
  for (int c = 1; c < nblk; ++c) if (last[c] < last[c - 1]) last[c] = last[c - 1];
  if (nblk >= 2 && last[nblk - 2] > nblk - 2) last[nblk - 2] = nblk - 2;
  return last;
}


void cholesky_envelope_bordered(const std::vector<int>& first_col, int border_begin, std::vector<int>* last_out, std::vector<int>* tail_out) {
  const int nblk = (int)first_col.size();
  const int bb = std::max(0, std::min(border_begin, nblk - 1));
  std::vector<int>& last = *last_out;
  std::vector<int>& tail = *tail_out;
  last.assign(nblk, 0); tail.assign(nblk, nblk - 1);
  // the band: rows before the border
  for (int c = 0; c < nblk; ++c) last[c] = c < bb ? c : nblk - 1;
  for (int i = 0; i < bb; ++i) { const int c = first_col[i] < i ? first_col[i] : i; if (c >= 0 && last[c] < i) last[c] = i; }
  for (int c = 1; c < bb; ++c) if (last[c] < last[c - 1]) last[c] = last[c - 1];
  // the border: row i is active from reach[i] on — its own first column, or that of any border row before it (a column's tail rows
  // are the LAST rows of the matrix: once row i is in, so is everything behind it); the right-hand-side row from column 0
  std::vector<int> reach(nblk, 0);
  int r = nblk;
  for (int i = bb; i < nblk - 1; ++i) { r = std::min(r, std::max(0, std::min(first_col[i], i))); reach[i] = r; }
  reach[nblk - 1] = 0;
  for (int c = 0; c < nblk; ++c) {  // first active border row of column c: reach is non-increasing in i, so the rows active in column c are a suffix
    int t = nblk - 1;
    while (t - 1 >= bb && reach[t - 1] <= c) --t;
    tail[c] = t;
  }
}

std::vector<int> cholesky_row_first_cols(int nblk, const int* last, const int* tail, int tail_rows) {
  std::vector<int> first(nblk, 0);
  if (!last) return first;
  int c0 = 0;
  for (int kb = 0; kb < nblk; ++kb) {  // last is non-decreasing: one sweep
    while (c0 < kb && last[c0] < kb) ++c0;
    first[kb] = c0;
  }
  if (tail) {
    for (int kb = 0; kb < nblk; ++kb) {  // ... or earlier, as a tail row (tail is non-increasing)
      int c = 0;
      while (c < first[kb] && tail[c] > kb) ++c;
      first[kb] = c;
    }
  } else {
    if (tail_rows < 1) tail_rows = 1;
    for (int kb = std::max(0, nblk - tail_rows); kb < nblk; ++kb) first[kb] = 0;
  }
  return first;
}

}  // namespace sk

// What tests/test_envelope_units_cpu.py holds against a brute-force block mask (a probe for the tests, not part of the C ABI of
// include/skeres_amd.h): active_rows[c * (nblk + 1) + r] = active_rows(c, r) for r in [0, nblk], height[c], the rows' first columns, the flops.
extern "C" void sk_envelope_probe(int nblk, const int* last, const int* tail, int ncols, int tail_rows, int* active_rows, int* height, int* row_first_cols,
                                  double* plan_flops) {
  const sk::BlockEnvelope env(nblk, last, tail, ncols, tail_rows);
  for (int c = 0; c < nblk; ++c) {
    for (int r = 0; r <= nblk; ++r) active_rows[c * (nblk + 1) + r] = env.active_rows(c, r);
    height[c] = env.height(c);
  }
  const std::vector<int> first = sk::cholesky_row_first_cols(nblk, last, tail, tail_rows);
  for (int i = 0; i < nblk; ++i) row_first_cols[i] = first[i];
  *plan_flops = sk::cholesky_plan_flops(nblk, last, ncols, tail_rows, tail);
}
