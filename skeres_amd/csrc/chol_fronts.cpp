// The fronts of sk_cholesky_solve* (chol_fronts.hpp).
#include "chol_fronts.hpp"

#include <cstdio>
#include <cstring>

namespace sk {

std::vector<int> host_block_first_cols(const std::vector<double>& M, size_t ld, int nblk) {
  std::vector<int> first_col(nblk);
  for (int i = 0; i < nblk; ++i) {
    first_col[i] = i;
    for (int j = 0; j < i && first_col[i] == i; ++j) {
      bool nz = false;
      for (int r = 0; r < 128 && !nz; ++r) {
        const double* row = &M[((size_t)i * 128 + r) * ld + (size_t)j * 128];
        for (int c = 0; c < 128; ++c) if (row[c] != 0.0) { nz = true; break; }
      }
      if (nz) first_col[i] = j;
    }
  }
  return first_col;
}
std::vector<int> host_block_envelope(const std::vector<double>& M, size_t ld, int nblk, int tail_rows) {
  return cholesky_envelope_last(host_block_first_cols(M, ld, nblk), tail_rows);
}

static std::string format(const char* fmt, int a, int b = 0, int c = 0) {
  char buf[160];
  std::snprintf(buf, sizeof buf, fmt, a, b, c);
  return buf;
}

// ---------------------------------------------------------------------------
// One front
// ---------------------------------------------------------------------------
int invalid_envelope_column(int n, const int* last) {
  const int nblk = single_front_blocks(n);
  for (int c = 0; c < nblk; ++c) {
    const bool ok = last[c] >= std::min(c, nblk - 2) && last[c] <= nblk - 1 && (c == 0 || last[c] >= last[c - 1]);
    if (!ok) return c;
  }
  return -1;
}

SingleFront single_front(int n, const double* A, const double* b, int border_begin_row) {
  SingleFront f;
  f.n = n; f.rhs_row = n; f.nblk = single_front_blocks(n); f.npad = f.nblk * 128;
  const int npad = f.npad, rhs_row = f.rhs_row;
  f.S.assign((size_t)npad * npad, 0.0);
  for (int i = 0; i < n; ++i) std::memcpy(&f.S[(size_t)i * npad], A + (size_t)i * n, (size_t)(i + 1) * sizeof(double));
  std::memcpy(&f.S[(size_t)rhs_row * npad], b, (size_t)n * sizeof(double));
  f.S[(size_t)rhs_row * npad + rhs_row] = 1e300;
  for (int j = n + 1; j < npad; ++j) f.S[(size_t)j * npad + j] = 1.0;
  if (border_begin_row >= 0) cholesky_envelope_bordered(host_block_first_cols(f.S, (size_t)npad, f.nblk), border_begin_row / 128, &f.last, &f.tail);
  return f;
}

void single_front_solution(const SingleFront& f, const std::vector<double>& y, double* x) { std::memcpy(x, y.data(), (size_t)f.n * sizeof(double)); }

void single_front_factor(const SingleFront& f, const std::vector<double>& S, double* L) {
  const int n = f.n;
  for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) L[(size_t)i * n + j] = j <= i ? S[(size_t)i * f.npad + j] : 0.0;
}

// ---------------------------------------------------------------------------
// Two-way dissection
// ---------------------------------------------------------------------------
std::string two_way_check(int n, const double* A, int head, int tail_begin) {
  for (int i = tail_begin; i < n; ++i)
    for (int j = 0; j < head; ++j)
      if (A[(size_t)i * n + j] != 0.0) return format("the tail couples with the head at (%d, %d): not a separator", i, j);
  return std::string();
}

TwoWayFronts two_way_fronts(int n, const double* A, const double* b, int head, int tail_begin) {
  TwoWayFronts f;
  const int ra = head, rb = tail_begin, nt = n - rb, msep = rb - ra;
  const int nA = (ra + 127) / 128, nB = (nt + 127) / 128, E = (msep + 1 + 127) / 128;
  const size_t dA = (size_t)(nA + E) * 128, dB = (size_t)(nB + E) * 128, dR = (size_t)E * 128;
  f.n = n; f.head = ra; f.tail_n = nt; f.sep_n = msep; f.border_blocks = E;
  std::vector<double>& FA = f.A.F; std::vector<double>& FB = f.B.F; std::vector<double>& FR = f.R.F;
  FA.assign(dA * dA, 0.0); FB.assign(dB * dB, 0.0); FR.assign(dR * dR, 0.0);
  // head: interior in order, border = separator in order, then the right-hand side
  for (int i = 0; i < ra; ++i) std::memcpy(&FA[(size_t)i * dA], A + (size_t)i * n, (size_t)(i + 1) * sizeof(double));
  for (int i = ra; i < nA * 128; ++i) FA[(size_t)i * dA + i] = 1.0;
  for (int k = 0; k < msep; ++k) std::memcpy(&FA[((size_t)nA * 128 + k) * dA], A + (size_t)(ra + k) * n, (size_t)ra * sizeof(double));
  std::memcpy(&FA[((size_t)nA * 128 + msep) * dA], b, (size_t)ra * sizeof(double));
  // tail: interior in REVERSE order (t <-> global n - 1 - t), border = separator in reverse order, then the right-hand side
  for (int t1 = 0; t1 < nt; ++t1)
    for (int t2 = 0; t2 <= t1; ++t2) FB[(size_t)t1 * dB + t2] = A[(size_t)(n - 1 - t2) * n + (n - 1 - t1)];
  for (int i = nt; i < nB * 128; ++i) FB[(size_t)i * dB + i] = 1.0;
  for (int k = 0; k < msep; ++k)
    for (int t = 0; t < nt; ++t) FB[((size_t)nB * 128 + k) * dB + t] = A[(size_t)(n - 1 - t) * n + (ra + msep - 1 - k)];
  for (int t = 0; t < nt; ++t) FB[((size_t)nB * 128 + msep) * dB + t] = b[n - 1 - t];
  // root: the separator's own block and right-hand side
  for (int i = 0; i < msep; ++i) std::memcpy(&FR[(size_t)i * dR], A + (size_t)(ra + i) * n + ra, (size_t)(i + 1) * sizeof(double));
  std::memcpy(&FR[(size_t)msep * dR], b + ra, (size_t)msep * sizeof(double));
  FR[(size_t)msep * dR + msep] = 1e300;
  for (size_t j = (size_t)msep + 1; j < dR; ++j) FR[j * dR + j] = 1.0;
  f.mapB.assign(dR, -1);
  for (int k = 0; k < msep; ++k) f.mapB[k] = msep - 1 - k;
  f.mapB[msep] = msep;
  f.A.dim = dA; f.A.nblk = nA + E; f.A.ncols = nA; f.A.rhs_row = nA * 128 + msep; f.A.last = host_block_envelope(FA, dA, nA + E);
  f.B.dim = dB; f.B.nblk = nB + E; f.B.ncols = nB; f.B.rhs_row = nB * 128 + msep; f.B.last = host_block_envelope(FB, dB, nB + E);
  f.R.dim = dR; f.R.nblk = E; f.R.ncols = E; f.R.rhs_row = msep;
  return f;
}

void two_way_scatter(const TwoWayFronts& f, const double* y, double* x) {
  for (int i = 0; i < f.head; ++i) x[i] = y[i];
  for (int t = 0; t < f.tail_n; ++t) x[f.n - 1 - t] = y[f.A.dim + t];
  for (int k = 0; k < f.sep_n; ++k) x[f.head + k] = y[f.A.dim + f.B.dim + k];
}

// ---------------------------------------------------------------------------
// Multi-way dissection
// ---------------------------------------------------------------------------
int SegmentCuts::root_index(int row) const {
  for (int k = 1; k < R; ++k) if (row >= sb[k] && row < se[k]) return sep_off[k - 1] + (row - sb[k]);
  return -1;
}

std::string segment_cuts(int n, const double* A, int R, const int* cuts, SegmentCuts* out) {
  SegmentCuts& c = *out;
  c.R = R; c.n = n;
  c.sb.assign(R + 1, 0); c.se.assign(R + 1, 0);
  std::vector<int>& sb = c.sb; std::vector<int>& se = c.se;
  sb[R] = n;
  for (int k = 1; k < R; ++k) { sb[k] = cuts[2 * (k - 1)]; se[k] = cuts[2 * (k - 1) + 1]; }
  for (int k = 1; k <= R; ++k)
    if (sb[k] < se[k - 1] || (k < R && (se[k] < sb[k] || se[k] > n))) return "invalid cuts";
  for (int k = 1; k < R; ++k)
    for (int i = se[k]; i < n; ++i)
      for (int j = 0; j < sb[k]; ++j)
        if (A[(size_t)i * n + j] != 0.0) return format("rows behind separator %d couple with rows before it at (%d, %d): not a separator", k, i, j);
  c.sep_off.assign(R, 0);
  for (int k = 1; k < R; ++k) c.sep_off[k] = c.sep_off[k - 1] + (se[k] - sb[k]);
  c.nroot = c.sep_off[R - 1];
  return std::string();
}

// (lower triangle given)
static inline double sym(const double* A, int n, int i, int j) { return i >= j ? A[(size_t)i * n + j] : A[(size_t)j * n + i]; }

HostFront segments_root(const SegmentCuts& c, const double* A, const double* b) {
  HostFront r;
  const int R = c.R, nroot = c.nroot, E = (nroot + 1 + 127) / 128;
  const size_t dR = (size_t)E * 128;
  r.dim = dR; r.nblk = E; r.ncols = E; r.rhs_row = nroot;
  std::vector<double>& FR = r.F;
  FR.assign(dR * dR, 0.0);
  for (int k = 1; k < R; ++k)
    for (int i = c.sb[k]; i < c.se[k]; ++i) {
      const int ri = c.root_index(i);
      for (int k2 = 1; k2 <= k; ++k2)
        for (int j = c.sb[k2]; j < c.se[k2] && j <= i; ++j) FR[(size_t)ri * dR + c.root_index(j)] = sym(A, c.n, i, j);
      FR[(size_t)nroot * dR + ri] = b[i];
    }
  FR[(size_t)nroot * dR + nroot] = 1e300;
  for (size_t j = (size_t)nroot + 1; j < dR; ++j) FR[j * dR + j] = 1.0;
  r.last = root_envelope(c.sep_off);
  return r;
}

LeafFront segment_leaf(const SegmentCuts& c, const double* A, const double* b, int k) {
  LeafFront f;
  const int R = c.R;
  const std::vector<int>& sb = c.sb; const std::vector<int>& se = c.se;
  const int lo = se[k], hi = sb[k + 1], ni = hi - lo;
  const int left_n = k > 0 ? se[k] - sb[k] : 0, right_n = k + 1 < R ? se[k + 1] - sb[k + 1] : 0;
  f.L = segment_layout(ni, left_n, right_n);
  f.interior_n = ni;
  const SegmentLayout& L = f.L;
  f.dim = (size_t)L.nblk * 128;
  const size_t d = f.dim;
  f.order.assign(d, -1);
  for (int t = 0; t < ni; ++t) f.order[t] = L.reversed ? hi - 1 - t : lo + t;
  const int bo = L.ncols * 128;
  if (L.right_off >= 0) for (int t = 0; t < right_n; ++t) f.order[bo + L.right_off + t] = sb[k + 1] + t;
  if (L.left_off >= 0) for (int t = 0; t < left_n; ++t) f.order[bo + L.left_off + t] = L.reversed ? se[k] - 1 - t : sb[k] + t;
  std::vector<double>& F = f.F;
  F.assign(d * d, 0.0);
  for (size_t i = 0; i < d; ++i) {
    const int gi = f.order[i];
    if (gi < 0) continue;
    for (size_t j = 0; j <= i && j < (size_t)ni; ++j) F[i * d + j] = sym(A, c.n, gi, f.order[j]);  // interior columns only: the border x border block starts at zero
  }
  for (int t = 0; t < ni; ++t) F[(size_t)L.rhs_row * d + t] = b[f.order[t]];
  for (int i = ni; i < bo; ++i) F[(size_t)i * d + i] = 1.0;
  f.last = host_block_envelope(F, d, L.nblk, L.tail_rows);
  f.map.assign(d - bo, -1);
  for (size_t i = bo; i < d; ++i) if (f.order[i] >= 0) f.map[i - bo] = c.root_index(f.order[i]);
  f.map[L.rhs_row - bo] = c.nroot;
  // border unknowns in the leaf's border order (zero in padding rows and in the right-hand-side row)
  f.gmap = f.map;
  f.gmap[L.rhs_row - bo] = -1;
  return f;
}

void segments_scatter_root(const SegmentCuts& c, const double* yR, double* x) {
  for (int k = 1; k < c.R; ++k) for (int i = c.sb[k]; i < c.se[k]; ++i) x[i] = yR[c.root_index(i)];
}

void segments_scatter_leaf(const LeafFront& f, const double* y, double* x) {
  for (int t = 0; t < f.L.ncols * 128; ++t) if (f.order[t] >= 0) x[f.order[t]] = y[t];
}

}  // namespace sk
