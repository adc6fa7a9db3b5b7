// Stand-alone check of the Schur-elimination part of the host-only covariance plan (skeres_amd/csrc/covariance_plan.cpp) on three
// synthetic problems: the chain of tools/covariance_plan_check.cpp (a hub, reversed neighbours, constant blocks), a small
// bundle-adjustment shape (a subset parameterization, a constant camera, a pair observed twice, a block that no residual block names,
// cameras that share hundreds of points: long Schur pairs) and one with a landmark seen by 150 cameras (a long (e, e) pair).  Verifies what the kernels rely on:
// E is independent and every F block has a neighbour in E or none at all; every pair is routed to the dense matrix or to a tile of
// its own, inside the buffers; F(e) lists the (g, e) tiles in ascending column order; every Schur term's tiles exist, belong to one
// e-block and to the pair's two F blocks, and each shared e-block appears once per pair, ascending; the parts tile the term lists;
// the selection contains F(e) for every requested e and every row range lies inside the k selected columns.
// Meant to be compiled with the host compiler under -fsanitize=address,undefined (no device code, no HIP):
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include tools/covariance_schur_plan_check.cpp \
//       skeres_amd/csrc/covariance_plan.cpp skeres_amd/csrc/jacobian_plan.cpp skeres_amd/csrc/evaluate_plan.cpp -o covariance_schur_plan_check && ./covariance_schur_plan_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../skeres_amd/csrc/covariance_plan.hpp"

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "covariance_schur_plan_check: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

using namespace sk;

namespace {
struct Builder {
  Problem p;
  std::vector<double> x;
  explicit Builder(size_t n) : x(n, 1.0) {}
  int block(size_t off, int size) {
    double* ptr = &x[off];
    auto it = p.block_of.find(ptr);
    if (it != p.block_of.end()) return it->second;
    const int id = (int)p.block_ptr.size();
    p.block_of.emplace(ptr, id); p.block_ptr.push_back(ptr); p.block_size.push_back(size);
    p.block_param.push_back(-1); p.block_constant.push_back(0);
    return id;
  }
  void add(int functor, int nres, std::vector<int> blocks) {
    p.rb_functor.push_back(functor); p.rb_num_residuals.push_back(nres); p.rb_const_off.push_back(p.consts.size());
    p.consts.push_back(0.5); p.consts.push_back(0.25); p.rb_cost.push_back(nullptr); p.rb_loss.push_back(-1);
    for (int b : blocks) p.rb_pidx.push_back(b);
    p.rb_pidx_off.push_back(p.rb_pidx.size());
    p.num_residuals += nres;
  }
};

int verify(const Problem& p, const std::vector<std::pair<int, int>>& pairs, const CovariancePlan& C) {
  const int ncb = (int)C.cols.cb_col.size(), npairs = (int)C.pair_i.size(), nE = C.num_elim;
  REQUIRE(C.schur && (int)C.cb_elim.size() == ncb && (int)C.cb_red.size() == ncb && (int)C.e_cb.size() == nE);
  // E is independent; the greedy rule restated: ascending (distinct neighbours, parameter block), join when no neighbour has joined
  std::vector<std::set<int>> nb(ncb);
  for (int q = 0; q < npairs; ++q) if (C.pair_i[q] != C.pair_j[q]) { nb[C.pair_i[q]].insert(C.pair_j[q]); nb[C.pair_j[q]].insert(C.pair_i[q]); }
  for (int q = 0; q < npairs; ++q) REQUIRE(C.pair_i[q] == C.pair_j[q] || !(C.cb_elim[C.pair_i[q]] && C.cb_elim[C.pair_j[q]]));
  std::vector<std::pair<size_t, int>> order;
  for (int c = 0; c < ncb; ++c) order.emplace_back(nb[c].size(), c);
  std::sort(order.begin(), order.end());
  std::vector<int> want(ncb, 0);
  for (const auto& oc : order) { bool free = true; for (int n : nb[oc.second]) free = free && !want[n]; want[oc.second] = free; }
  for (int c = 0; c < ncb; ++c) REQUIRE(want[c] == C.cb_elim[c]);
  // the reduced columns and the e-block indices
  int red = 0, e = 0;
  for (int c = 0; c < ncb; ++c) {
    if (C.cb_elim[c]) { REQUIRE(C.cb_red[c] == e && C.e_cb[e] == c); ++e; }
    else { REQUIRE(C.cb_red[c] == red); red += C.cols.cb_size[c]; }
  }
  REQUIRE(e == nE && red == C.red_cols && red <= kCovarianceMaxColumns);
  // the routing: every pair to the dense matrix or to one tile; tiles are distinct and inside the buffer
  REQUIRE((int)C.pair_tile.size() == npairs && (int)C.pair_flip.size() == npairs && C.num_tiles >= 2 * nE);
  std::set<int> tiles;
  std::map<std::pair<int, int>, int> tile_of;  // (g, e as column blocks) -> tile
  for (int q = 0; q < npairs; ++q) {
    const int i = C.pair_i[q], j = C.pair_j[q], t = C.pair_tile[q];
    if (!C.cb_elim[i] && !C.cb_elim[j]) { REQUIRE(t == -1); REQUIRE(C.cb_red[i] + C.cols.cb_size[i] <= C.red_cols && C.cb_red[j] + C.cols.cb_size[j] <= C.red_cols); continue; }
    REQUIRE(t >= 0 && t < C.num_tiles && tiles.insert(t).second);
    if (i == j) { REQUIRE(t == C.cb_red[i] && !C.pair_flip[q]); continue; }
    REQUIRE(t >= 2 * nE && C.pair_flip[q] == C.cb_elim[i]);
    tile_of[{C.pair_flip[q] ? j : i, C.pair_flip[q] ? i : j}] = t;
  }
  REQUIRE(C.num_tiles == 2 * nE + (int)tile_of.size());
  // F(e): the (g, e) tiles in ascending order of g
  REQUIRE((int)C.ew_begin.size() == nE + 1 && C.ew_begin[0] == 0 && C.ew_begin[nE] == (int)tile_of.size());
  REQUIRE(C.ew_tile.size() == tile_of.size() && C.ew_g.size() == tile_of.size() && C.ew_sel.size() == tile_of.size());
  std::vector<int> e_of_tile(C.num_tiles, -1), g_of_tile(C.num_tiles, -1);
  long long terms = 0;
  for (e = 0; e < nE; ++e) {
    const int n = C.ew_begin[e + 1] - C.ew_begin[e];
    REQUIRE(n == (int)nb[C.e_cb[e]].size());
    terms += (long long)n * (n + 1) / 2;
    for (int k = C.ew_begin[e]; k < C.ew_begin[e + 1]; ++k) {
      REQUIRE(k == C.ew_begin[e] || C.ew_g[k - 1] < C.ew_g[k]);
      auto it = tile_of.find({C.ew_g[k], C.e_cb[e]});
      REQUIRE(it != tile_of.end() && it->second == C.ew_tile[k] && !C.cb_elim[C.ew_g[k]]);
      e_of_tile[C.ew_tile[k]] = e; g_of_tile[C.ew_tile[k]] = C.ew_g[k];
    }
  }
  REQUIRE(terms == C.schur_terms && terms == (long long)C.st_a.size() && C.st_b.size() == C.st_a.size() && C.st_ne.size() == C.st_a.size());
  // the Schur terms: per pair (g >= g') one term per shared e-block, ascending; every tile exists and is the pair's
  const int nsp = (int)C.sp_i.size();
  REQUIRE((int)C.sp_begin.size() == nsp + 1 && C.sp_begin[nsp] == (int)terms);
  for (int q = 0; q < nsp; ++q) {
    const int g = C.sp_i[q], h = C.sp_j[q];
    REQUIRE(g >= h && !C.cb_elim[g] && !C.cb_elim[h] && (q == 0 || C.sp_i[q - 1] < g || (C.sp_i[q - 1] == g && C.sp_j[q - 1] < h)));
    REQUIRE(C.sp_begin[q + 1] > C.sp_begin[q]);
    int shared = 0;
    for (int n : nb[g]) shared += C.cb_elim[n] && (g == h || nb[h].count(n));
    REQUIRE(shared == C.sp_begin[q + 1] - C.sp_begin[q]);
    for (int k = C.sp_begin[q]; k < C.sp_begin[q + 1]; ++k) {
      const int a = C.st_a[k], b = C.st_b[k];
      REQUIRE(a >= 2 * nE && a < C.num_tiles && b >= 2 * nE && b < C.num_tiles && g_of_tile[a] == g && g_of_tile[b] == h);
      REQUIRE(e_of_tile[a] >= 0 && e_of_tile[a] == e_of_tile[b] && C.st_ne[k] == C.cols.cb_size[C.e_cb[e_of_tile[a]]]);
      REQUIRE(k == C.sp_begin[q] || e_of_tile[C.st_a[k - 1]] < e_of_tile[a]);
    }
  }
  // the parts tile the term lists
  const int nparts = (int)C.schur_parts.owner.size();
  int part = 0, partial = 0, nlong = 0;
  for (int q = 0; q < nsp; ++q) {
    const int begin = C.sp_begin[q], end = C.sp_begin[q + 1], first = part;
    int at = begin;
    do {
      REQUIRE(part < nparts && C.schur_parts.owner[part] == q && C.schur_parts.begin[part] == at);
      REQUIRE(C.schur_parts.end[part] == (at + kCgnrPartSlots < end ? at + kCgnrPartSlots : end));
      at = C.schur_parts.end[part++];
    } while (at < end);
    if (part - first == 1) { REQUIRE(C.schur_parts.out[first] == -1); continue; }
    REQUIRE(C.schur_parts.long_owner[nlong] == q && C.schur_parts.long_begin[nlong] == partial);
    for (int k = first; k < part; ++k) REQUIRE(C.schur_parts.out[k] == partial++);
    REQUIRE(C.schur_parts.long_begin[++nlong] == partial);
  }
  REQUIRE(part == nparts && partial == C.schur_parts.num_partials && nlong == (int)C.schur_parts.long_owner.size() && (int)C.schur_parts.long_begin.size() == nlong + 1);
  // the selection: F blocks only, columns of the reduced matrix; a requested e-block has all of F(e) selected
  std::vector<int> cb_of(p.block_ptr.size(), -1), sel_row(ncb, -1);
  for (int c = 0; c < ncb; ++c) cb_of[C.cols.cb_block[c]] = c;
  REQUIRE(C.sel_off.size() == C.sel_cb.size() + 1 && C.k == (int)C.sel_col.size() && C.sel_off.back() == C.k);
  for (size_t i = 0; i < C.sel_cb.size(); ++i) {
    const int c = C.sel_cb[i];
    REQUIRE(!C.cb_elim[c] && sel_row[c] < 0 && C.sel_off[i + 1] - C.sel_off[i] == C.cols.cb_size[c]);
    sel_row[c] = C.sel_off[i];
    for (int j = 0; j < C.cols.cb_size[c]; ++j) REQUIRE(C.sel_col[C.sel_off[i] + j] == C.cb_red[c] + j && C.sel_col[C.sel_off[i] + j] < C.red_cols);
  }
  std::set<int> requested_e;
  REQUIRE(C.req_ea.size() == C.req_a.size() && C.req_eb.size() == C.req_a.size());
  for (size_t r = 0; r < C.req_a.size(); ++r) {
    const int side[2] = {C.req_a[r], C.req_b[r]}, row[2] = {C.req_ra[r], C.req_rb[r]}, eb[2] = {C.req_ea[r], C.req_eb[r]};
    const bool zero = cb_of[side[0]] < 0 || cb_of[side[1]] < 0;
    for (int t = 0; t < 2; ++t) {
      if (zero) { REQUIRE(row[t] == -1 && eb[t] == -1); continue; }
      const int c = cb_of[side[t]];
      if (C.cb_elim[c]) { REQUIRE(eb[t] == C.cb_red[c] && row[t] >= 0); requested_e.insert(eb[t]); }
      else REQUIRE(eb[t] == -1 && row[t] == sel_row[c] && row[t] >= 0 && row[t] + C.cols.cb_size[c] <= C.k);
    }
  }
  for (e = 0; e < nE; ++e)
    for (int k = C.ew_begin[e]; k < C.ew_begin[e + 1]; ++k) {
      if (requested_e.count(e)) REQUIRE(C.ew_sel[k] == sel_row[C.ew_g[k]] && C.ew_sel[k] >= 0 && C.ew_sel[k] + C.cols.cb_size[C.ew_g[k]] <= C.k);
      else REQUIRE(C.ew_sel[k] == -1);
    }
  return 0;
}
}  // namespace

int main() {
  std::string why;
  {  // the chain
    const int nblocks = 2100, hub = 7, hub_blocks = 320;
    Builder B(2 * nblocks);
    auto blk = [&](int b) { return B.block(2 * (size_t)b, 2); };
    for (int i = 0; i + 1 < nblocks; ++i) { if (i % 5 == 0) B.add(SK_FUNCTOR_BINARY_VECTOR3_COST, 3, {blk(i + 1), blk(i)}); else B.add(SK_FUNCTOR_BINARY_VECTOR3_COST, 3, {blk(i), blk(i + 1)}); }
    for (int k = 0; k < hub_blocks; ++k) { const int j = 20 + 6 * k; if (k % 2 == 0) B.add(SK_FUNCTOR_BINARY_VECTOR3_COST, 3, {blk(hub), blk(j)}); else B.add(SK_FUNCTOR_BINARY_VECTOR3_COST, 3, {blk(j), blk(hub)}); }
    B.p.block_constant[blk(100)] = 1; B.p.block_constant[blk(101)] = 1;
    const std::vector<std::pair<int, int>> pairs = {{blk(hub), blk(0)}, {blk(nblocks - 1), blk(hub)}, {blk(6), blk(5)}, {blk(5), blk(6)}, {blk(100), blk(hub)}, {blk(20), blk(20)}};
    CovariancePlan C;
    REQUIRE(covariance_plan_build(B.p, pairs, &C, &why, true) == SK_OK);
    REQUIRE(verify(B.p, pairs, C) == 0);
    int hub_cb = -1;
    for (size_t c = 0; c < C.cols.cb_block.size(); ++c) if (C.cols.cb_block[c] == blk(hub)) hub_cb = (int)c;
    REQUIRE(hub_cb >= 0 && !C.cb_elim[hub_cb]);   // the hub has the most neighbours: visited last, and a neighbour has joined
    printf("covariance_schur_plan_check chain ok: %d columns, %d eliminated blocks, %d reduced columns, %lld Schur terms, %zu parts, k = %d\n", C.cols.num_cols, C.num_elim,
           C.red_cols, C.schur_terms, C.schur_parts.owner.size(), C.k);
  }
  {  // a bundle-adjustment shape: 5 cameras of 9, 400 points of 3, three observations per point, one pair observed twice
    const int ncam = 5, npt = 400;
    Builder B(9 * ncam + 3 * npt + 4);
    auto cam = [&](int c) { return B.block(9 * (size_t)c, 9); };
    auto pt = [&](int q) { return B.block(9 * (size_t)ncam + 3 * (size_t)q, 3); };
    for (int q = 0; q < npt; ++q) for (int t = 0; t < 3; ++t) B.add(SK_FUNCTOR_SNAVELY_REPROJECTION, 2, {cam((q + t) % ncam), pt(q)});
    B.add(SK_FUNCTOR_SNAVELY_REPROJECTION, 2, {cam(1), pt(0)});
    const int lone = B.block(9 * (size_t)ncam + 3 * (size_t)npt, 4);
    B.p.block_constant[cam(0)] = 1;
    LocalParameterization subset; subset.type = kParamSubset; subset.global_size = 9; subset.local_size = 6; subset.constant_mask = 0x1c0u;
    B.p.params.push_back(subset);
    B.p.block_param[cam(2)] = 0;
    const std::vector<std::pair<int, int>> pairs = {{pt(0), cam(1)}, {cam(2), cam(2)}, {cam(2), cam(3)}, {cam(0), cam(2)}, {lone, lone}, {pt(7), pt(0)}, {pt(7), pt(7)}};
    CovariancePlan C;
    REQUIRE(covariance_plan_build(B.p, pairs, &C, &why, true) == SK_OK);
    REQUIRE(verify(B.p, pairs, C) == 0);
    REQUIRE(C.num_elim == npt + 1 && C.red_cols == 9 * 3 + 6);   // the points and the block that nothing names
    REQUIRE(!C.schur_parts.long_owner.empty() && C.schur_parts.num_partials > 0);       // two cameras share more than 64 points
    printf("covariance_schur_plan_check bundle-adjustment shape ok: %d columns, %d eliminated blocks, %d reduced columns, %lld Schur terms, k = %d\n", C.cols.num_cols,
           C.num_elim, C.red_cols, C.schur_terms, C.k);
  }
  {  // a landmark: 150 cameras, 400 points in windows of 4, point 400 seen by every camera
    const int ncam = 150, npt = 401;
    Builder B(9 * ncam + 3 * npt);
    auto cam = [&](int c) { return B.block(9 * (size_t)c, 9); };
    auto pt = [&](int q) { return B.block(9 * (size_t)ncam + 3 * (size_t)q, 3); };
    for (int q = 0; q + 1 < npt; ++q) for (int t = 0; t < 4; ++t) B.add(SK_FUNCTOR_SNAVELY_REPROJECTION, 2, {cam((7 * q + t) % ncam), pt(q)});
    for (int c = 0; c < ncam; ++c) B.add(SK_FUNCTOR_SNAVELY_REPROJECTION, 2, {cam(c), pt(npt - 1)});
    B.p.block_constant[cam(0)] = 1; B.p.block_constant[cam(1)] = 1;
    const std::vector<std::pair<int, int>> pairs = {{pt(npt - 1), pt(npt - 1)}, {pt(npt - 1), pt(3)}, {cam(5), pt(npt - 1)}, {cam(5), cam(90)}, {cam(0), pt(3)}};
    CovariancePlan C;
    REQUIRE(covariance_plan_build(B.p, pairs, &C, &why, true) == SK_OK);
    REQUIRE(verify(B.p, pairs, C) == 0);
    REQUIRE(C.num_elim == npt && C.red_cols == 9 * (ncam - 2) && C.k == 9 * (ncam - 2));   // the landmark selects every moving camera
    REQUIRE(!C.pair_parts.long_owner.empty());   // the landmark's own (e, e) pair: 150 terms
    printf("covariance_schur_plan_check landmark ok: %d columns, %d reduced columns, %lld Schur terms, %zu long Schur pairs, %d partial tiles, k = %d\n", C.cols.num_cols,
           C.red_cols, C.schur_terms, C.schur_parts.long_owner.size(), C.schur_parts.num_partials, C.k);
  }
  {  // refusals: the column cap counts what is left; the default's message points at the setter
    Builder B(16 * 2049);
    for (int i = 0; i < 2049; ++i) B.block(16 * (size_t)i, 16);
    REQUIRE(covariance_refusal(B.p).find("sk_covariance_options_set_schur_elimination") != std::string::npos && covariance_refusal(B.p, true).empty());
    CovariancePlan C;
    REQUIRE(covariance_plan_build(B.p, {{0, 0}}, &C, &why, true) == SK_OK && C.red_cols == 0 && C.num_elim == 2049 && C.k == 0);
    Builder P(16 * 4100);
    for (int i = 0; i + 1 < 4100; ++i) P.add(SK_FUNCTOR_BINARY_VECTOR3_COST, 3, {P.block(16 * (size_t)i, 16), P.block(16 * (size_t)(i + 1), 16)});
    const int rc = covariance_plan_build(P.p, {{0, 0}}, &C, &why, true);
    REQUIRE(rc == SK_ERR_UNSUPPORTED && why.find("after the elimination") != std::string::npos && why.find("32800") != std::string::npos);
    printf("covariance_schur_plan_check refusals ok\n");
  }
  return 0;
}
