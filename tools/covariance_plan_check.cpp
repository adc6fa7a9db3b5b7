// Stand-alone check of the host-only covariance plan (skeres_amd/csrc/covariance_plan.cpp) on three synthetic problems: the chain
// of tools/cgnr_plan_check.cpp (a hub whose diagonal pair is six parts, reversed neighbours, constant blocks), a small
// bundle-adjustment shape (cameras of 9 with a subset parameterization, points of 3, a constant camera, a (camera, point) pair
// observed twice, a block that no residual block names) and a problem above the column cap.  Verifies what the kernels rely on: every
// stored pair of slots of every residual block is a term of exactly one pair, in row order; the parts tile the term lists; the
// selection and the requested pairs index the k x k result and the packed output without overlap.
// Meant to be compiled with the host compiler under -fsanitize=address,undefined (no device code, no HIP):
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include tools/covariance_plan_check.cpp \
//       skeres_amd/csrc/covariance_plan.cpp skeres_amd/csrc/jacobian_plan.cpp skeres_amd/csrc/evaluate_plan.cpp -o covariance_plan_check && ./covariance_plan_check
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "../skeres_amd/csrc/covariance_plan.hpp"

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "covariance_plan_check: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

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

// the plan against a brute-force enumeration of the problem's structure
int verify(const Problem& p, const std::vector<std::pair<int, int>>& pairs, const CovariancePlan& C) {
  const EvaluatePlan& E = C.eval;
  const int num_pb = (int)p.block_ptr.size(), ncb = (int)C.cols.cb_col.size(), nb = (int)E.blocks.size(), npairs = (int)C.pair_i.size();
  // columns
  int cols = 0;
  std::vector<int> cb_of(num_pb, -1);
  for (int c = 0; c < ncb; ++c) {
    const int b = C.cols.cb_block[c];
    REQUIRE(b >= 0 && b < num_pb && !p.block_constant[b] && C.cols.cb_col[c] == cols && C.cols.cb_size[c] == E.col_size[b] && C.cols.cb_size[c] > 0 && C.cols.cb_size[c] <= kCovarianceMaxBlock);
    REQUIRE(C.cols.pb_local_off[b] == cols && (c == 0 || C.cols.cb_block[c - 1] < b));
    cb_of[b] = c; cols += C.cols.cb_size[c];
  }
  REQUIRE(cols == C.cols.num_cols);
  for (int b = 0; b < num_pb; ++b) REQUIRE((cb_of[b] >= 0) == (C.cols.pb_local_off[b] >= 0) && (cb_of[b] >= 0 || p.block_constant[b] || E.col_size[b] == 0));
  // terms: the brute-force lists per (i, j), in row order
  std::map<std::pair<int, int>, std::vector<std::pair<int, int>>> want;
  for (int i = 0; i < nb; ++i)
    for (int s = E.slot_begin[i]; s < E.slot_begin[i + 1]; ++s)
      for (int t = E.slot_begin[i]; t < E.slot_begin[i + 1]; ++t) {
        if (E.slot_pos[s] < 0 || E.slot_pos[t] < 0) continue;
        const int ci = cb_of[E.slot_block[s]], cj = cb_of[E.slot_block[t]];
        REQUIRE(ci >= 0 && cj >= 0);
        if (ci >= cj) want[{ci, cj}].emplace_back(s, t);
      }
  REQUIRE((int)want.size() == npairs && (int)C.pair_begin.size() == npairs + 1 && C.pair_begin[npairs] == (int)C.term_si.size());
  int q = 0;
  for (const auto& kv : want) {   // (the map's order is the plan's: by i, then j)
    REQUIRE(C.pair_i[q] == kv.first.first && C.pair_j[q] == kv.first.second && C.cols.cb_col[C.pair_i[q]] >= C.cols.cb_col[C.pair_j[q]]);
    REQUIRE(C.pair_begin[q + 1] - C.pair_begin[q] == (int)kv.second.size());
    for (size_t k = 0; k < kv.second.size(); ++k) {
      const int si = C.term_si[C.pair_begin[q] + k], sj = C.term_sj[C.pair_begin[q] + k];
      REQUIRE(si == kv.second[k].first && sj == kv.second[k].second && E.slot_owner[si] == E.slot_owner[sj]);
      const int i = E.slot_owner[si], nres = E.row_off[i + 1] - E.row_off[i], width = (E.val_off[i + 1] - E.val_off[i]) / nres;
      REQUIRE(E.slot_pos[si] + C.cols.cb_size[C.pair_i[q]] <= width && E.slot_pos[sj] + C.cols.cb_size[C.pair_j[q]] <= width && E.val_off[i + 1] <= E.num_nonzeros);
    }
    ++q;
  }
  // parts
  const int nparts = (int)C.pair_parts.owner.size();
  int part = 0, partial = 0, nlong = 0;
  for (q = 0; q < npairs; ++q) {
    const int begin = C.pair_begin[q], end = C.pair_begin[q + 1], first = part;
    REQUIRE(end > begin);
    int at = begin;
    do {
      REQUIRE(part < nparts && C.pair_parts.owner[part] == q && C.pair_parts.begin[part] == at);
      REQUIRE(C.pair_parts.end[part] == (at + kCgnrPartSlots < end ? at + kCgnrPartSlots : end));
      at = C.pair_parts.end[part++];
    } while (at < end);
    if (part - first == 1) { REQUIRE(C.pair_parts.out[first] == -1); continue; }
    REQUIRE(C.pair_parts.long_owner[nlong] == q && C.pair_parts.long_begin[nlong] == partial);
    for (int k = first; k < part; ++k) REQUIRE(C.pair_parts.out[k] == partial++);
    REQUIRE(C.pair_parts.long_begin[++nlong] == partial);
  }
  REQUIRE(part == nparts && partial == C.pair_parts.num_partials && nlong == (int)C.pair_parts.long_owner.size() && (int)C.pair_parts.long_begin.size() == nlong + 1);
  // the selection: moving blocks named by the pairs, in order of first appearance; columns inside H
  std::vector<int> order;
  for (const auto& ab : pairs)
    for (int b : {ab.first, ab.second}) {
      bool seen = false;
      for (int o : order) seen = seen || o == b;
      if (!seen && cb_of[b] >= 0) order.push_back(b);
    }
  REQUIRE(order.size() == C.sel_cb.size() && C.sel_off.size() == order.size() + 1 && C.k == (int)C.sel_col.size() && C.sel_off.back() == C.k);
  for (size_t i = 0; i < order.size(); ++i) {
    REQUIRE(C.sel_cb[i] == cb_of[order[i]] && C.sel_off[i + 1] - C.sel_off[i] == C.cols.cb_size[C.sel_cb[i]]);
    for (int j = 0; j < C.cols.cb_size[C.sel_cb[i]]; ++j) REQUIRE(C.sel_col[C.sel_off[i] + j] == C.cols.cb_col[C.sel_cb[i]] + j && C.sel_col[C.sel_off[i] + j] < C.cols.num_cols);
  }
  // the requested pairs: each unordered pair once; blocks of the packed output do not overlap and fill it
  std::map<std::pair<int, int>, int> once;
  long at = 0;
  for (size_t r = 0; r < C.req_a.size(); ++r) {
    const int a = C.req_a[r], b = C.req_b[r];
    REQUIRE(a <= b && once.emplace(std::make_pair(a, b), 1).second);
    const bool zero = cb_of[a] < 0 || cb_of[b] < 0;
    REQUIRE((C.req_ra[r] < 0) == zero && (C.req_rb[r] < 0) == zero);
    if (!zero) {
      REQUIRE(C.req_ra[r] + E.col_size[a] <= C.k && C.req_rb[r] + E.col_size[b] <= C.k);
      REQUIRE(C.sel_col[C.req_ra[r]] == C.cols.pb_local_off[a] && C.sel_col[C.req_rb[r]] == C.cols.pb_local_off[b]);
    }
    REQUIRE(C.req_tan_off[r] == at); at += (long)E.col_size[a] * E.col_size[b];
    REQUIRE(C.req_amb_off[r] == at); at += (long)p.block_size[a] * p.block_size[b];
    REQUIRE(E.col_size[a] * E.col_size[b] <= kCovarianceTile && p.block_size[a] * p.block_size[b] <= kCovarianceTile);
  }
  REQUIRE(at == C.out_size);
  for (const auto& ab : pairs) REQUIRE(once.count({ab.first < ab.second ? ab.first : ab.second, ab.first < ab.second ? ab.second : ab.first}) == 1);
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
    REQUIRE(covariance_refusal(B.p).empty());
    const std::vector<std::pair<int, int>> pairs = {{blk(hub), blk(0)}, {blk(nblocks - 1), blk(hub)}, {blk(6), blk(5)}, {blk(5), blk(6)}, {blk(hub), blk(0)}, {blk(100), blk(hub)}, {blk(100), blk(100)}};
    CovariancePlan C;
    REQUIRE(covariance_plan_build(B.p, pairs, &C, &why) == SK_OK);
    REQUIRE(verify(B.p, pairs, C) == 0);
    REQUIRE(C.cols.num_cols == 2 * (nblocks - 2) && C.k == 10 && C.req_a.size() == 5);          // hub, 0, last, 6, 5; the duplicates and the swap collapse
    REQUIRE(C.pair_parts.long_owner.size() == 1 && C.pair_parts.num_partials == (hub_blocks + 2 + kCgnrPartSlots - 1) / kCgnrPartSlots);   // the hub's diagonal: 320 + its two neighbours
    printf("covariance_plan_check chain ok: %d columns, %zu pairs, %zu terms, %zu parts, %d partial tiles, k = %d\n", C.cols.num_cols, C.pair_i.size(), C.term_si.size(),
           C.pair_parts.owner.size(), C.pair_parts.num_partials, C.k);
  }
  {  // a bundle-adjustment shape: 5 cameras of 9, 40 points of 3, three observations per point, one pair observed twice
    const int ncam = 5, npt = 40;
    Builder B(9 * ncam + 3 * npt + 4);
    auto cam = [&](int c) { return B.block(9 * (size_t)c, 9); };
    auto pt = [&](int q) { return B.block(9 * (size_t)ncam + 3 * (size_t)q, 3); };
    for (int q = 0; q < npt; ++q) for (int t = 0; t < 3; ++t) B.add(SK_FUNCTOR_SNAVELY_REPROJECTION, 2, {cam((q + t) % ncam), pt(q)});
    B.add(SK_FUNCTOR_SNAVELY_REPROJECTION, 2, {cam(1), pt(0)});   // (camera 1, point 0) a second time
    const int lone = B.block(9 * (size_t)ncam + 3 * (size_t)npt, 4);     // in the problem, in no residual block
    B.p.block_constant[cam(0)] = 1;
    LocalParameterization subset; subset.type = kParamSubset; subset.global_size = 9; subset.local_size = 6; subset.constant_mask = 0x1c0u;
    B.p.params.push_back(subset);
    B.p.block_param[cam(2)] = 0;
    REQUIRE(covariance_refusal(B.p).empty());
    const std::vector<std::pair<int, int>> pairs = {{pt(0), cam(1)}, {cam(2), cam(2)}, {cam(2), cam(3)}, {cam(0), cam(2)}, {lone, lone}, {pt(7), pt(0)}};
    CovariancePlan C;
    REQUIRE(covariance_plan_build(B.p, pairs, &C, &why) == SK_OK);
    REQUIRE(verify(B.p, pairs, C) == 0);
    REQUIRE(C.cols.num_cols == 9 * 3 + 6 + 3 * npt + 4 && C.k == 3 + 9 + 6 + 9 + 4 + 3);
    bool two_terms = false;
    for (size_t q = 0; q < C.pair_i.size(); ++q)
      two_terms = two_terms || (C.cols.cb_block[C.pair_i[q]] == cam(1) && C.cols.cb_block[C.pair_j[q]] == pt(0) && C.pair_begin[q + 1] - C.pair_begin[q] == 2);   // (point 0 was named first: the lower column)
    REQUIRE(two_terms);
    for (size_t q = 0; q < C.pair_i.size(); ++q) REQUIRE(C.cols.cb_block[C.pair_i[q]] != lone);   // no pair: its diagonal stays zero, and the device flags it
    printf("covariance_plan_check bundle-adjustment shape ok: %d columns, %zu pairs, %zu terms, k = %d\n", C.cols.num_cols, C.pair_i.size(), C.term_si.size(), C.k);
    const std::vector<std::pair<int, int>> bad = {{0, (int)B.p.block_ptr.size()}};
    REQUIRE(covariance_plan_build(B.p, bad, &C, &why) == SK_ERR_INVALID_ARGUMENT);
  }
  {  // above the cap, a block above 16, dense rows
    Builder B(16 * 2049);
    for (int i = 0; i < 2049; ++i) B.block(16 * (size_t)i, 16);
    const std::string r = covariance_refusal(B.p);
    REQUIRE(r.find("32768") != std::string::npos && r.find("32784") != std::string::npos && r.find("not built") != std::string::npos);
    CovariancePlan C;
    REQUIRE(covariance_plan_build(B.p, {{0, 0}}, &C, &why) == SK_ERR_UNSUPPORTED && why == r);
    Builder W(17);
    W.block(0, 17);
    REQUIRE(covariance_refusal(W.p).find("tangent size") != std::string::npos);
    Builder D(4);
    D.add(SK_FUNCTOR_SYNTH_TANH_ROW, 1, {D.block(0, 4)});
    REQUIRE(covariance_refusal(D.p).find("dense-row") != std::string::npos);
    printf("covariance_plan_check refusals ok\n");
  }
  return 0;
}
