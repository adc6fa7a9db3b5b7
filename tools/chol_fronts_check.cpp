// Stand-alone check of the front layouts of sk_cholesky_solve* (skeres_amd/csrc/chol_fronts.cpp): SPD systems with the sparsity the
// plans are for — block-banded segments with separators between them, diagonally dominant, fixed seeds — are laid out as the device
// unit lays them out, and what the device calls do to the fronts is carried out here in plain host arithmetic: the partial Cholesky
// of a leaf's interior columns, its border x border Schur complement added to the root through `map` (the right-hand side travels as
// a matrix row: it is w = L^-1 b after the factorisation), the root's factorisation and solve, the gather through `gmap`, the leaf's
// back-substitution y_i = L_ii^-T (w_i - L_bi^T y_b), the scatter into x.  x is held against a direct solve of the system by
//
//   |A x - b|_inf <= c n u (|A|_inf |x|_inf + |b|_inf),   c = 8 x what the DIRECT solve of the same system leaves of that ratio
//
// (the fronts are the same Cholesky in another elimination order: the factor 8 is the room for that; nothing the layouts produce
// enters the bound; the residuals are formed in extended precision).  Beside it the structure: orders
// are permutations, every separator row is in the root once, the right-hand side's map entries, every non-zero of a front and of
// its factor inside the front's envelope, the padding rows.
// Meant to be compiled with the host compiler under -fsanitize=address,undefined (no device code, no HIP):
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/chol_fronts_check.cpp \
//       skeres_amd/csrc/chol_fronts.cpp skeres_amd/csrc/chol_envelope.cpp -o chol_fronts_check && ./chol_fronts_check
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../skeres_amd/csrc/chol_fronts.hpp"

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "chol_fronts_check: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

using namespace sk;

// ---------------------------------------------------------------------------
// Systems
// ---------------------------------------------------------------------------
struct System {
  std::string name;
  int n = 0;
  std::vector<int> cuts;  // (begin, end) of each separator
  std::vector<double> A, b;  // A: n x n, lower triangle
  int segments() const { return (int)cuts.size() / 2 + 1; }
};

// Segment k's rows couple within a band of 30; separator k couples with itself, with the last 40 rows of the segment before it, the
// first 40 of the one behind it and with the separator before it.
static System make_system(const std::string& name, const std::vector<int>& interiors, const std::vector<int>& seps, uint64_t seed) {
  System s;
  s.name = name;
  const int R = (int)interiors.size();
  std::vector<int> kind, lo_of, hi_of;  // kind: 2 k segment k, 2 k - 1 separator k
  for (int k = 0; k < R; ++k) {
    if (k > 0) { s.cuts.push_back(s.n); for (int t = 0; t < seps[k - 1]; ++t) kind.push_back(2 * k - 1); s.n += seps[k - 1]; s.cuts.push_back(s.n); }
    for (int t = 0; t < interiors[k]; ++t) kind.push_back(2 * k);
    s.n += interiors[k];
  }
  const int n = s.n;
  lo_of.assign(2 * R, n); hi_of.assign(2 * R, 0);
  for (int i = 0; i < n; ++i) { lo_of[kind[i]] = std::min(lo_of[kind[i]], i); hi_of[kind[i]] = std::max(hi_of[kind[i]], i + 1); }
  auto next = [&seed] { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (double)(seed >> 11) / 9007199254740992.0 * 2.0 - 1.0; };
  s.A.assign((size_t)n * n, 0.0); s.b.assign(n, 0.0);
  std::vector<double> row_sum(n, 0.0);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < i; ++j) {
      const int ki = kind[i], kj = kind[j];
      bool on = false;
      if (ki == kj) on = ki % 2 == 1 || i - j <= 30;
      else if (ki % 2 == 1 && kj == ki - 1) on = j >= hi_of[kj] - 40;  // separator x the segment before it
      else if (kj % 2 == 1 && ki == kj + 1) on = i < lo_of[ki] + 40;   // the segment behind a separator x the separator
      else if (ki % 2 == 1 && kj == ki - 2) on = true;                 // separator x the separator before it
      if (!on) continue;
      const double v = next();
      s.A[(size_t)i * n + j] = v;
      row_sum[i] += std::fabs(v); row_sum[j] += std::fabs(v);
    }
  for (int i = 0; i < n; ++i) { s.A[(size_t)i * n + i] = 1.0 + row_sum[i]; s.b[i] = next(); }
  return s;
}

// ---------------------------------------------------------------------------
// Host arithmetic on a front (row-major lower triangle, d x d)
// ---------------------------------------------------------------------------
// Cholesky of the first nc columns in place: the rows below them solved, the trailing block reduced by their Schur complement.
// (By rows' first non-zero columns: a row has no fill before its first entry, so the skipped products are exact zeros.)
static bool partial_cholesky(std::vector<double>& F, size_t d, size_t nc) {
  std::vector<size_t> first(d);
  for (size_t i = 0; i < d; ++i) { first[i] = 0; while (first[i] < i && F[i * d + first[i]] == 0.0) ++first[i]; }
  for (size_t j = 0; j < nc; ++j)
    for (size_t i = j; i < d; ++i) {
      if (first[i] > j) continue;
      double s = F[i * d + j];
      for (size_t k = std::max(first[i], first[j]); k < j; ++k) s -= F[i * d + k] * F[j * d + k];
      if (i == j) { if (!(s > 0.0)) return false; F[j * d + j] = std::sqrt(s); }
      else F[i * d + j] = s / F[j * d + j];
    }
  for (size_t i = nc; i < d; ++i)
    for (size_t j = nc; j <= i; ++j) {
      double s = 0.0;
      for (size_t k = std::max(first[i], first[j]); k < nc; ++k) s += F[i * d + k] * F[j * d + k];
      F[i * d + j] -= s;
    }
  return true;
}
// y = L^-T w over the first m rows of a factored front
static void back_substitute(const std::vector<double>& F, size_t d, size_t m, std::vector<double> w, double* y) {
  for (size_t i = m; i-- > 0;) {
    y[i] = w[i] / F[i * d + i];
    for (size_t k = 0; k < i; ++k) w[k] -= F[i * d + k] * y[i];
  }
}
// every non-zero in the first ncols block columns lies inside the envelope
static bool inside_envelope(const std::vector<double>& F, size_t d, const BlockEnvelope& env) {
  for (size_t i = 0; i < d; ++i)
    for (size_t j = 0; j <= i && j < (size_t)env.ncols * 128; ++j) {
      if (F[i * d + j] == 0.0) continue;
      const int bi = (int)(i / 128), bj = (int)(j / 128);
      if (bi != bj && bi > env.last_row(bj) && bi < env.tail_begin(bj)) return false;
    }
  return true;
}
// rows [from, to) are rows and columns of the identity
static bool identity_rows(const std::vector<double>& F, size_t d, size_t from, size_t to) {
  for (size_t i = from; i < to; ++i) {
    for (size_t j = 0; j < i; ++j) if (F[i * d + j] != 0.0) return false;
    if (F[i * d + i] != 1.0) return false;
    for (size_t r = i + 1; r < d; ++r) if (F[r * d + i] != 0.0) return false;
  }
  return true;
}
static bool zero_row(const std::vector<double>& F, size_t d, size_t i) {
  for (size_t j = 0; j <= i; ++j) if (F[i * d + j] != 0.0) return false;
  return true;
}

// A leaf as the device sees it: the partial factorisation, the border added to the root through map, the back-substitution with the
// border's unknowns gathered through gmap.
struct Leaf { std::vector<double> F; size_t d = 0; int ncols = 0, rhs_row = 0; std::vector<int> map, gmap; std::vector<double> y; };

static bool eliminate_into_root(Leaf& l, std::vector<double>& root, size_t dR) {
  if (l.ncols == 0) return true;
  const size_t bo = (size_t)l.ncols * 128;
  if (!partial_cholesky(l.F, l.d, bo)) return false;
  for (size_t i = 0; i < l.d - bo; ++i)
    for (size_t j = 0; j <= i; ++j) {
      const int ri = l.map[i], rj = l.map[j];
      if (ri < 0 || rj < 0) continue;
      root[(size_t)std::max(ri, rj) * dR + std::min(ri, rj)] += l.F[(bo + i) * l.d + bo + j];
    }
  return true;
}
static void solve_leaf(Leaf& l, const std::vector<double>& yR) {
  const size_t bo = (size_t)l.ncols * 128;
  l.y.assign(l.d, 0.0);
  if (l.ncols == 0) return;
  std::vector<double> w(bo);
  for (size_t c = 0; c < bo; ++c) w[c] = l.F[(size_t)l.rhs_row * l.d + c];
  for (size_t r = 0; r < l.d - bo; ++r) {
    const double yb = l.gmap[r] >= 0 ? yR[l.gmap[r]] : 0.0;
    for (size_t c = 0; c < bo; ++c) w[c] -= l.F[(bo + r) * l.d + c] * yb;
  }
  back_substitute(l.F, l.d, bo, w, l.y.data());
}
// the root once every leaf is in it: factored whole, solved for its first nroot rows
static bool solve_root(std::vector<double>& FR, size_t dR, int nroot, std::vector<double>* yR) {
  if (!partial_cholesky(FR, dR, dR)) return false;
  yR->assign(dR, 0.0);
  std::vector<double> w(nroot);
  for (int c = 0; c < nroot; ++c) w[c] = FR[(size_t)nroot * dR + c];
  back_substitute(FR, dR, nroot, w, yR->data());
  return true;
}

// ---------------------------------------------------------------------------
// The yardstick
// ---------------------------------------------------------------------------
// |A x - b|_inf / (n u (|A|_inf |x|_inf + |b|_inf)), the residual in extended precision
static double residual_ratio(const System& s, const std::vector<double>& x) {
  const int n = s.n;
  double rmax = 0.0, anorm = 0.0, xnorm = 0.0, bnorm = 0.0;
  for (int i = 0; i < n; ++i) {
    long double r = -(long double)s.b[i];
    double rowsum = 0.0;
    for (int j = 0; j < n; ++j) {
      const double a = i >= j ? s.A[(size_t)i * n + j] : s.A[(size_t)j * n + i];
      r += (long double)a * x[j];
      rowsum += std::fabs(a);
    }
    rmax = std::max(rmax, (double)fabsl(r)); anorm = std::max(anorm, rowsum);
    xnorm = std::max(xnorm, std::fabs(x[i])); bnorm = std::max(bnorm, std::fabs(s.b[i]));
  }
  return rmax / (n * (std::numeric_limits<double>::epsilon() / 2) * (anorm * xnorm + bnorm));
}
static bool direct_solve(const System& s, std::vector<double>* x) {
  const size_t n = s.n;
  std::vector<double> L(s.A), w(s.b);
  if (!partial_cholesky(L, n, n)) return false;
  for (size_t i = 0; i < n; ++i) { for (size_t k = 0; k < i; ++k) w[i] -= L[i * n + k] * w[k]; w[i] /= L[i * n + i]; }
  x->assign(n, 0.0);
  back_substitute(L, n, n, w, x->data());
  return true;
}

// ---------------------------------------------------------------------------
// The three shapes
// ---------------------------------------------------------------------------
static int single(const System& s, int border_begin_row, std::vector<double>* x) {
  const int n = s.n;
  SingleFront f = single_front(n, s.A.data(), s.b.data(), border_begin_row);
  REQUIRE(f.n == n && f.rhs_row == n && f.nblk == single_front_blocks(n) && f.npad == f.nblk * 128 && f.npad > n && f.S.size() == (size_t)f.npad * f.npad);
  REQUIRE(f.S[(size_t)n * f.npad + n] == 1e300 && identity_rows(f.S, f.npad, n + 1, f.npad));
  const std::vector<int> dense(f.nblk, f.nblk - 1);
  REQUIRE(invalid_envelope_column(n, dense.data()) == -1);
  if (border_begin_row >= 0) {
    REQUIRE((int)f.last.size() == f.nblk && (int)f.tail.size() == f.nblk);
    REQUIRE(inside_envelope(f.S, f.npad, BlockEnvelope(f.nblk, f.last.data(), f.tail.data())));
  } else {
    REQUIRE(f.last.empty() && f.tail.empty());
  }
  REQUIRE(partial_cholesky(f.S, f.npad, f.npad));
  if (border_begin_row >= 0) REQUIRE(inside_envelope(f.S, f.npad, BlockEnvelope(f.nblk, f.last.data(), f.tail.data())));
  std::vector<double> w(n), y(f.npad, 0.0), L((size_t)n * n, -1.0);
  for (int c = 0; c < n; ++c) w[c] = f.S[(size_t)f.rhs_row * f.npad + c];
  back_substitute(f.S, f.npad, n, w, y.data());
  x->assign(n, 0.0);
  single_front_solution(f, y, x->data());
  single_front_factor(f, f.S, L.data());
  for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) REQUIRE(L[(size_t)i * n + j] == (j <= i ? f.S[(size_t)i * f.npad + j] : 0.0));
  return 0;
}

static int two_way(const System& s, std::vector<double>* x) {
  const int n = s.n, head = s.cuts[0], tail_begin = s.cuts[1], msep = tail_begin - head, nt = n - tail_begin;
  REQUIRE(two_way_check(n, s.A.data(), head, tail_begin).empty());
  const TwoWayFronts f = two_way_fronts(n, s.A.data(), s.b.data(), head, tail_begin);
  const int E = (msep + 1 + 127) / 128;
  REQUIRE(f.n == n && f.head == head && f.tail_n == nt && f.sep_n == msep && f.border_blocks == E);
  REQUIRE(f.A.ncols == (head + 127) / 128 && f.A.nblk == f.A.ncols + E && f.A.dim == (size_t)f.A.nblk * 128 && f.A.rhs_row == f.A.ncols * 128 + msep);
  REQUIRE(f.B.ncols == (nt + 127) / 128 && f.B.nblk == f.B.ncols + E && f.B.dim == (size_t)f.B.nblk * 128 && f.B.rhs_row == f.B.ncols * 128 + msep);
  REQUIRE(f.R.ncols == E && f.R.nblk == E && f.R.dim == (size_t)E * 128 && f.R.rhs_row == msep && f.R.last.empty());
  REQUIRE(f.A.F.size() == f.A.dim * f.A.dim && f.B.F.size() == f.B.dim * f.B.dim && f.R.F.size() == f.R.dim * f.R.dim);
  REQUIRE((int)f.A.last.size() == f.A.nblk && (int)f.B.last.size() == f.B.nblk && f.mapB.size() == f.R.dim);
  // the tail's border is the separator reversed; the right-hand side goes to the root's
  std::vector<int> seen(msep, 0);
  for (size_t i = 0; i < f.mapB.size(); ++i) {
    if ((int)i < msep) { REQUIRE(f.mapB[i] == msep - 1 - (int)i); ++seen[f.mapB[i]]; }
    else REQUIRE(f.mapB[i] == ((int)i == msep ? msep : -1));
  }
  for (int k = 0; k < msep; ++k) REQUIRE(seen[k] == 1);
  REQUIRE(f.R.F[(size_t)msep * f.R.dim + msep] == 1e300 && identity_rows(f.R.F, f.R.dim, msep + 1, f.R.dim));
  const HostFront* hf[2] = {&f.A, &f.B};
  const int interior[2] = {head, nt};
  Leaf leaf[2];
  for (int q = 0; q < 2; ++q) {
    const HostFront& h = *hf[q];
    const size_t bo = (size_t)h.ncols * 128;
    REQUIRE(identity_rows(h.F, h.dim, interior[q], bo));
    for (size_t i = bo + msep + 1; i < h.dim; ++i) REQUIRE(zero_row(h.F, h.dim, i));
    for (size_t i = bo; i < h.dim; ++i) for (size_t j = bo; j <= i; ++j) REQUIRE(h.F[i * h.dim + j] == 0.0);  // the border x border block starts at zero
    const BlockEnvelope env(h.nblk, h.last.data(), nullptr, h.ncols);
    REQUIRE(inside_envelope(h.F, h.dim, env));
    Leaf& l = leaf[q];
    l.F = h.F; l.d = h.dim; l.ncols = h.ncols; l.rhs_row = h.rhs_row;
    l.map.assign(h.dim - bo, -1); l.gmap.assign(h.dim - bo, -1);
    for (size_t i = 0; i < l.map.size(); ++i) l.map[i] = q == 0 ? (int)i : f.mapB[i];  // (the head's border is in the root's order)
    for (int i = 0; i < msep; ++i) l.gmap[i] = l.map[i];
  }
  std::vector<double> FR(f.R.F), yR;
  for (int q = 0; q < 2; ++q) {
    REQUIRE(eliminate_into_root(leaf[q], FR, f.R.dim));
    REQUIRE(inside_envelope(leaf[q].F, leaf[q].d, BlockEnvelope(hf[q]->nblk, hf[q]->last.data(), nullptr, hf[q]->ncols)));
  }
  REQUIRE(solve_root(FR, f.R.dim, msep, &yR));
  std::vector<double> y;
  for (int q = 0; q < 2; ++q) { solve_leaf(leaf[q], yR); y.insert(y.end(), leaf[q].y.begin(), leaf[q].y.end()); }
  y.insert(y.end(), yR.begin(), yR.end());
  x->assign(n, std::numeric_limits<double>::quiet_NaN());
  two_way_scatter(f, y.data(), x->data());
  return 0;
}

static int multi_way(const System& s, std::vector<double>* x) {
  const int n = s.n, R = s.segments();
  SegmentCuts c;
  REQUIRE(segment_cuts(n, s.A.data(), R, s.cuts.data(), &c).empty());
  REQUIRE(c.R == R && c.n == n && (int)c.sb.size() == R + 1 && (int)c.se.size() == R + 1 && (int)c.sep_off.size() == R && c.se[0] == 0 && c.sb[R] == n);
  // every separator row is in the root once, nothing else is
  std::vector<int> in_root(c.nroot, 0), is_sep(n, 0);
  for (int k = 1; k < R; ++k) {
    REQUIRE(c.sb[k] == s.cuts[2 * (k - 1)] && c.se[k] == s.cuts[2 * (k - 1) + 1] && c.sep_off[k] - c.sep_off[k - 1] == c.se[k] - c.sb[k]);
    for (int i = c.sb[k]; i < c.se[k]; ++i) is_sep[i] = 1;
  }
  REQUIRE(c.nroot == c.sep_off[R - 1]);
  for (int i = 0; i < n; ++i) {
    const int r = c.root_index(i);
    if (!is_sep[i]) { REQUIRE(r == -1); continue; }
    REQUIRE(r >= 0 && r < c.nroot);
    ++in_root[r];
  }
  for (int r = 0; r < c.nroot; ++r) REQUIRE(in_root[r] == 1);
  const HostFront root = segments_root(c, s.A.data(), s.b.data());
  const int nroot = c.nroot;
  REQUIRE(root.nblk == (nroot + 1 + 127) / 128 && root.ncols == root.nblk && root.dim == (size_t)root.nblk * 128 && root.rhs_row == nroot && root.F.size() == root.dim * root.dim);
  REQUIRE(root.F[(size_t)nroot * root.dim + nroot] == 1e300 && identity_rows(root.F, root.dim, nroot + 1, root.dim));
  REQUIRE(root.last.empty() || (int)root.last.size() == root.nblk);
  const BlockEnvelope renv(root.nblk, root.last.empty() ? nullptr : root.last.data());
  REQUIRE(inside_envelope(root.F, root.dim, renv));
  std::vector<double> FR(root.F), yR;
  std::vector<Leaf> leaves(R);
  std::vector<LeafFront> fronts(R);
  std::vector<int> covered(n, 0);
  for (int k = 0; k < R; ++k) {
    fronts[k] = segment_leaf(c, s.A.data(), s.b.data(), k);
    const LeafFront& f = fronts[k];
    const SegmentLayout& L = f.L;
    const int lo = c.se[k], hi = c.sb[k + 1], ni = hi - lo, bo = L.ncols * 128;
    const int left_n = k > 0 ? c.se[k] - c.sb[k] : 0, right_n = k + 1 < R ? c.se[k + 1] - c.sb[k + 1] : 0;
    const size_t d = f.dim;
    REQUIRE(f.interior_n == ni && L.ncols == (ni + 127) / 128 && d == (size_t)L.nblk * 128 && f.F.size() == d * d && f.order.size() == d);
    REQUIRE(f.map.size() == d - bo && f.gmap.size() == d - bo && (int)f.last.size() == L.nblk);
    REQUIRE(L.spike == (left_n > 0 && right_n > 0) &&(L.spike || L.tail_rows == 1) && L.rhs_row >= bo && L.rhs_row < (int)d);
    // order: the segment's rows, each once, then padding up to the border
    std::vector<int> hits(ni, 0);
    for (int t = 0; t < bo; ++t) {
      if (t >= ni) { REQUIRE(f.order[t] == -1); continue; }
      REQUIRE(f.order[t] >= lo && f.order[t] < hi);
      ++hits[f.order[t] - lo]; ++covered[f.order[t]];
    }
    for (int t = 0; t < ni; ++t) REQUIRE(hits[t] == 1);
    // the border: the two separators beside the segment, each row once; map and gmap
    std::vector<int> border_hits(nroot, 0);
    int border_rows = 0;
    for (size_t i = bo; i < d; ++i) {
      const int g = f.order[i], bi = (int)(i - bo);
      if ((int)i == L.rhs_row) { REQUIRE(g == -1 && f.map[bi] == nroot && f.gmap[bi] == -1); continue; }
      if (g < 0) { REQUIRE(f.map[bi] == -1 && f.gmap[bi] == -1 && zero_row(f.F, d, i)); continue; }  // padding in a border: zero
      REQUIRE((k > 0 && g >= c.sb[k] && g < c.se[k]) || (k + 1 < R && g >= c.sb[k + 1] && g < c.se[k + 1]));
      REQUIRE(f.map[bi] == c.root_index(g) && f.gmap[bi] == f.map[bi]);
      ++border_hits[f.map[bi]]; ++border_rows;
    }
    REQUIRE(border_rows == left_n + right_n);
    for (int r = 0; r < nroot; ++r) REQUIRE(border_hits[r] <= 1);
    REQUIRE(identity_rows(f.F, d, ni, bo));
    for (size_t i = bo; i < d; ++i) for (size_t j = bo; j <= i; ++j) REQUIRE(f.F[i * d + j] == 0.0);
    const BlockEnvelope env(L.nblk, f.last.data(), nullptr, L.ncols, L.tail_rows);
    REQUIRE(env.tail_rows == L.tail_rows && inside_envelope(f.F, d, env));
    Leaf& l = leaves[k];
    l.F = f.F; l.d = d; l.ncols = L.ncols; l.rhs_row = L.rhs_row; l.map = f.map; l.gmap = f.gmap;
    REQUIRE(eliminate_into_root(l, FR, root.dim));
    REQUIRE(inside_envelope(l.F, d, env));
  }
  for (int i = 0; i < n; ++i) REQUIRE(covered[i] + is_sep[i] == 1);
  REQUIRE(inside_envelope(FR, root.dim, renv));
  REQUIRE(solve_root(FR, root.dim, nroot, &yR));
  REQUIRE(inside_envelope(FR, root.dim, renv));
  x->assign(n, std::numeric_limits<double>::quiet_NaN());
  segments_scatter_root(c, yR.data(), x->data());
  for (int k = 0; k < R; ++k) { solve_leaf(leaves[k], yR); segments_scatter_leaf(fronts[k], leaves[k].y.data(), x->data()); }
  return 0;
}

// the refusals and their messages
static int refusals() {
  const System s = make_system("refusals", {130, 140, 100}, {10, 17}, 77);
  const int n = s.n;
  std::vector<int> last(single_front_blocks(n), single_front_blocks(n) - 1);
  last[1] = 0;
  REQUIRE(invalid_envelope_column(n, last.data()) == 1);
  last[1] = single_front_blocks(n);
  REQUIRE(invalid_envelope_column(n, last.data()) == 1);
  std::vector<double> A(s.A);
  A[(size_t)300 * n + 5] = 0.5;
  REQUIRE(two_way_check(n, A.data(), 130, 297) == "the tail couples with the head at (300, 5): not a separator");
  REQUIRE(two_way_check(n, A.data(), 5, 297).empty());
  SegmentCuts c;
  REQUIRE(segment_cuts(n, A.data(), 3, s.cuts.data(), &c) == "rows behind separator 1 couple with rows before it at (300, 5): not a separator");
  for (const std::vector<int>& bad : {std::vector<int>{140, 130, 280, 297}, std::vector<int>{130, 290, 280, 297}, std::vector<int>{130, 140, 280, n + 1}, std::vector<int>{-1, 140, 280, 297}})
    REQUIRE(segment_cuts(n, s.A.data(), 3, bad.data(), &c) == "invalid cuts");
  return 0;
}

int main() {
  struct Case { System s; int shape, border_begin_row; };  // shape: 1 one front, 2 two-way, 3 multi-way
  std::vector<Case> cases;
  cases.push_back({make_system("single n=127", {127}, {}, 1), 1, -1});
  cases.push_back({make_system("single n=128", {128}, {}, 2), 1, -1});
  cases.push_back({make_system("single n=129", {129}, {}, 3), 1, -1});
  cases.push_back({make_system("single n=300 bordered at 200", {200, 0}, {100}, 4), 1, 200});
  cases.push_back({make_system("two-way 130|20|150", {130, 150}, {20}, 5), 2, -1});
  cases.push_back({make_system("two-way 0|20|150", {0, 150}, {20}, 6), 2, -1});
  cases.push_back({make_system("two-way 130|20|0", {130, 0}, {20}, 7), 2, -1});
  cases.push_back({make_system("two-way 130|0|150", {130, 150}, {0}, 8), 2, -1});
  cases.push_back({make_system("two-way 130|127|150", {130, 150}, {127}, 9), 2, -1});
  cases.push_back({make_system("two-way 130|128|150", {130, 150}, {128}, 10), 2, -1});
  cases.push_back({make_system("multi-way 130|10|140|17|100", {130, 140, 100}, {10, 17}, 11), 3, -1});
  cases.push_back({make_system("multi-way 130|10|0|17|100", {130, 0, 100}, {10, 17}, 12), 3, -1});
  cases.push_back({make_system("multi-way 130|10|60|17|70|5|100", {130, 60, 70, 100}, {10, 17, 5}, 13), 3, -1});
  cases.push_back({make_system("multi-way 130|10|140|128|100", {130, 140, 100}, {10, 128}, 14), 3, -1});
  // the two-way systems through the multi-way layout as well (R = 2: the head and the tail of the two-way case)
  for (size_t k = 4; k < 10; ++k) { Case c = cases[k]; c.s.name = "multi-way R=2 of " + c.s.name; c.shape = 3; cases.push_back(c); }
  if (refusals()) return 1;
  double direct_max = 0.0;
  std::vector<double> direct(cases.size());
  for (size_t k = 0; k < cases.size(); ++k) {
    std::vector<double> xd;
    REQUIRE(direct_solve(cases[k].s, &xd));
    direct[k] = residual_ratio(cases[k].s, xd);
    direct_max = std::max(direct_max, direct[k]);
  }
  double fronts_max = 0.0;
  for (size_t k = 0; k < cases.size(); ++k) {
    const Case& c = cases[k];
    std::vector<double> x;
    if (c.shape == 1 ? single(c.s, c.border_begin_row, &x) : c.shape == 2 ? two_way(c.s, &x) : multi_way(c.s, &x)) { fprintf(stderr, "chol_fronts_check: in %s\n", c.s.name.c_str()); return 1; }
    for (double v : x) REQUIRE(std::isfinite(v));
    const double ratio = residual_ratio(c.s, x), c_bound = 8.0 * direct[k];
    printf("%-44s n %3d  residual ratio: fronts %.4f  direct %.4f  (c = 8 x that = %.4f)\n", c.s.name.c_str(), c.s.n, ratio, direct[k], c_bound);
    fronts_max = std::max(fronts_max, ratio);
    if (!(ratio <= c_bound)) { fprintf(stderr, "chol_fronts_check: %s misses the residual bound\n", c.s.name.c_str()); return 1; }
  }
  printf("chol_fronts_check ok: %zu systems, largest residual ratio of the fronts %.4f, of the direct solves %.4f\n", cases.size(), fronts_max, direct_max);
  return 0;
}
