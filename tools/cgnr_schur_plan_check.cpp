// Stand-alone check of the Schur elimination of the host-only CGNR plan (skeres_amd/csrc/cgnr_plan.cpp): builds the plan with the
// elimination for two structures — the chain of tools/cgnr_plan_check.cpp (2100 blocks of size 2, every fifth pair reversed, a hub in
// 320 more residual blocks, two constant blocks) and a bundle-adjustment shape (5 cameras of size 9, one of them constant; 150
// points of size 3, one seen by all cameras 20 times over: a long e-block; one observation repeated) — and verifies what the kernels
// rely on.  Meant to be compiled with the host compiler under -fsanitize=address,undefined (no device code, no HIP):
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include tools/cgnr_schur_plan_check.cpp \
//       skeres_amd/csrc/cgnr_plan.cpp skeres_amd/csrc/jacobian_plan.cpp skeres_amd/csrc/evaluate_plan.cpp -o cgnr_schur_plan_check && ./cgnr_schur_plan_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../skeres_amd/csrc/cgnr_plan.hpp"

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "cgnr_schur_plan_check: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

using namespace sk;

namespace {

struct Builder {
  Problem p;
  std::vector<double> x;
  std::vector<int> off;
  explicit Builder(const std::vector<int>& sizes) {
    off.push_back(0);
    for (int s : sizes) off.push_back(off.back() + s);
    x.assign(off.back(), 1.0);
    for (size_t b = 0; b < sizes.size(); ++b) {   // (registered in this order: the parameter-block index is the index here)
      p.block_of.emplace(&x[off[b]], (int)b); p.block_ptr.push_back(&x[off[b]]); p.block_size.push_back(sizes[b]);
      p.block_param.push_back(-1); p.block_constant.push_back(0);
    }
  }
  void add(int functor, int nres, int nconsts, int a, int b) {
    p.rb_functor.push_back(functor); p.rb_num_residuals.push_back(nres); p.rb_const_off.push_back(p.consts.size());
    for (int k = 0; k < nconsts; ++k) p.consts.push_back(0.5);
    p.rb_cost.push_back(nullptr); p.rb_loss.push_back(-1);
    p.rb_pidx.push_back(a); p.rb_pidx.push_back(b); p.rb_pidx_off.push_back(p.rb_pidx.size());
    p.num_residuals += nres;
  }
};

// What every plan with the elimination must satisfy.  Returns 0, or the line of the failed requirement.
int check(const Problem& p, const CgnrPlan& C, const CgnrPlan& plain) {
  const EvaluatePlan& E = C.eval;
  const TangentColumns& T = C.cols;
  const int ncb = (int)T.cb_col.size(), ns = (int)E.slot_block.size(), nb = (int)E.blocks.size();
  // the plan without the elimination is a prefix: same columns, slot lists and parts
  REQUIRE(C.cb_begin == plain.cb_begin && C.cb_slots == plain.cb_slots && C.slot_size == plain.slot_size && C.parts.owner == plain.parts.owner);
  REQUIRE(plain.cb_elim.empty() && plain.F.cb.empty() && plain.E.cb.empty() && plain.fp_e.empty() && plain.slot_size_f.empty() && plain.fp_begin.empty());
  REQUIRE((int)C.cb_elim.size() == ncb);
  // E is independent: no residual block names two e-blocks
  std::vector<std::set<int>> nbrs(ncb);
  for (int i = 0; i < nb; ++i) {
    for (int s = E.slot_begin[i]; s < E.slot_begin[i + 1]; ++s) {
      if (E.slot_pos[s] < 0) continue;
      const int c = T.cb_of[E.slot_block[s]];
      for (int t = E.slot_begin[i]; t < E.slot_begin[i + 1]; ++t) if (E.slot_pos[t] >= 0 && T.cb_of[E.slot_block[t]] != c) nbrs[c].insert(T.cb_of[E.slot_block[t]]);
    }
    std::set<int> es;
    for (int s = E.slot_begin[i]; s < E.slot_begin[i + 1]; ++s) if (E.slot_pos[s] >= 0 && C.cb_elim[T.cb_of[E.slot_block[s]]]) es.insert(T.cb_of[E.slot_block[s]]);
    REQUIRE(es.size() <= 1);
  }
  // the greedy rule itself, restated: ascending (distinct neighbours, column block)
  {
    std::vector<int> order(ncb), want(ncb, 0);
    for (int c = 0; c < ncb; ++c) order[c] = c;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return nbrs[a].size() < nbrs[b].size(); });
    for (int c : order) { bool free = true; for (int q : nbrs[c]) if (want[q]) free = false; want[c] = free; }
    REQUIRE(want == C.cb_elim);
  }
  // F and E partition the column blocks; each subset's lists are the full plan's, its parts tile them
  int reduced = 0;
  for (int pass = 0; pass < 2; ++pass) {
    const CgnrColumnSubset& S = pass ? C.E : C.F;
    REQUIRE(S.cb_begin.size() == S.cb.size() + 1 && S.cb_col.size() == S.cb.size() && S.cb_size.size() == S.cb.size() && S.cb_moff.size() == S.cb.size());
    for (size_t k = 0; k < S.cb.size(); ++k) {
      const int c = S.cb[k];
      REQUIRE(c >= 0 && c < ncb && C.cb_elim[c] == pass && (k == 0 || S.cb[k - 1] < c));
      REQUIRE(S.cb_col[k] == T.cb_col[c] && S.cb_size[k] == T.cb_size[c] && S.cb_moff[k] == C.cb_moff[c]);
      REQUIRE(S.cb_begin[k + 1] - S.cb_begin[k] == C.cb_begin[c + 1] - C.cb_begin[c]);
      for (int j = 0; j < S.cb_begin[k + 1] - S.cb_begin[k]; ++j) REQUIRE(S.cb_slots[S.cb_begin[k] + j] == C.cb_slots[C.cb_begin[c] + j]);
      if (!pass) reduced += T.cb_size[c];
    }
    int part = 0, partial = 0, nlong = 0;
    for (size_t k = 0; k < S.cb.size(); ++k) {
      int at = S.cb_begin[k];
      const int end = S.cb_begin[k + 1], first = part;
      do {
        REQUIRE(part < (int)S.parts.owner.size() && S.parts.owner[part] == (int)k && S.parts.begin[part] == at);
        REQUIRE(S.parts.end[part] == std::min(at + kCgnrPartSlots, end));
        at = S.parts.end[part++];
      } while (at < end);
      if (part - first == 1) { REQUIRE(S.parts.out[first] == -1); continue; }
      REQUIRE(S.parts.long_owner[nlong] == (int)k && S.parts.long_begin[nlong] == partial);
      for (int q = first; q < part; ++q) REQUIRE(S.parts.out[q] == partial++);
      REQUIRE(S.parts.long_begin[++nlong] == partial);
    }
    REQUIRE(part == (int)S.parts.owner.size() && partial == S.parts.num_partials && nlong == (int)S.parts.long_owner.size());
  }
  REQUIRE((int)(C.F.cb.size() + C.E.cb.size()) == ncb && reduced == C.reduced_cols);
  REQUIRE(C.F.parts.num_partials <= C.parts.num_partials);   // (the partial sums of J_F^T w fit the full plan's buffer)
  // slot_size_f: 0 exactly on E's stored slots
  REQUIRE((int)C.slot_size_f.size() == ns);
  for (int s = 0; s < ns; ++s) {
    const bool in_e = E.slot_pos[s] >= 0 && C.cb_elim[T.cb_of[E.slot_block[s]]];
    REQUIRE(C.slot_size_f[s] == (in_e ? 0 : C.slot_size[s]));
  }
  // the pairs: per F block its distinct e-neighbours ascending; the terms of a pair in row order, both slots of one residual
  // block, g's slot on g and e's slot on e; every (F slot, E slot) of every residual block exactly once
  const int nf = (int)C.F.cb.size(), npairs = (int)C.fp_e.size();
  REQUIRE((int)C.fp_begin.size() == nf + 1 && C.fp_begin[0] == 0 && C.fp_begin[nf] == npairs && (int)C.fp_slot_begin.size() == npairs + 1);
  REQUIRE(C.fp_slot_g.size() == C.fp_slot_e.size() && C.fp_slot_begin[0] == 0 && C.fp_slot_begin[npairs] == (int)C.fp_slot_g.size());
  std::set<std::pair<int, int>> seen;
  for (int f = 0; f < nf; ++f) {
    std::set<int> es;
    for (int q = C.fp_begin[f]; q < C.fp_begin[f + 1]; ++q) {
      const int e = C.fp_e[q];
      REQUIRE(e >= 0 && e < ncb && C.cb_elim[e] && (q == C.fp_begin[f] || C.fp_e[q - 1] < e));
      es.insert(e);
      REQUIRE(C.fp_slot_begin[q] < C.fp_slot_begin[q + 1]);
      for (int k = C.fp_slot_begin[q]; k < C.fp_slot_begin[q + 1]; ++k) {
        const int sg = C.fp_slot_g[k], se = C.fp_slot_e[k];
        REQUIRE(sg >= 0 && sg < ns && se >= 0 && se < ns && E.slot_pos[sg] >= 0 && E.slot_pos[se] >= 0 && E.slot_owner[sg] == E.slot_owner[se]);
        REQUIRE(T.cb_of[E.slot_block[sg]] == C.F.cb[f] && T.cb_of[E.slot_block[se]] == e);
        REQUIRE(k == C.fp_slot_begin[q] || E.slot_owner[C.fp_slot_g[k - 1]] <= E.slot_owner[sg]);
        REQUIRE(seen.emplace(sg, se).second);
      }
    }
    std::set<int> want;
    for (int q : nbrs[C.F.cb[f]]) if (C.cb_elim[q]) want.insert(q);
    REQUIRE(es == want);
  }
  size_t want_terms = 0;
  for (int i = 0; i < nb; ++i) {
    int fs = 0, es = 0;
    for (int s = E.slot_begin[i]; s < E.slot_begin[i + 1]; ++s) if (E.slot_pos[s] >= 0) (C.cb_elim[T.cb_of[E.slot_block[s]]] ? es : fs)++;
    want_terms += (size_t)fs * es;
  }
  REQUIRE(seen.size() == want_terms);
  // the parts of the pair lists
  {
    const PartList& L = C.fp_parts;
    int part = 0;
    for (int f = 0; f < nf; ++f) {
      int at = C.fp_begin[f];
      do {
        REQUIRE(part < (int)L.owner.size() && L.owner[part] == f && L.begin[part] == at && L.end[part] == std::min(at + kCgnrPartSlots, C.fp_begin[f + 1]));
        at = L.end[part++];
      } while (at < C.fp_begin[f + 1]);
    }
    REQUIRE(part == (int)L.owner.size());
  }
  (void)p;
  return 0;
}

}  // namespace

int main() {
  // the chain
  {
    const int nblocks = 2100, hub = 7, hub_blocks = 320;
    Builder B(std::vector<int>(nblocks, 2));
    for (int i = 0; i + 1 < nblocks; ++i) { if (i % 5 == 0) B.add(SK_FUNCTOR_BINARY_VECTOR3_COST, 3, 1, i + 1, i); else B.add(SK_FUNCTOR_BINARY_VECTOR3_COST, 3, 1, i, i + 1); }
    for (int k = 0; k < hub_blocks; ++k) { const int j = 20 + 6 * k; if (k % 2 == 0) B.add(SK_FUNCTOR_BINARY_VECTOR3_COST, 3, 1, hub, j); else B.add(SK_FUNCTOR_BINARY_VECTOR3_COST, 3, 1, j, hub); }
    B.p.block_constant[100] = 1; B.p.block_constant[101] = 1;
    REQUIRE(cgnr_refusal(B.p, 1, false).empty());
    CgnrPlan C, plain;
    std::string why;
    REQUIRE(cgnr_plan_build(B.p, &plain, &why) == SK_OK && cgnr_plan_build(B.p, &C, &why, true) == SK_OK);
    const int rc = check(B.p, C, plain);
    if (rc) return rc;
    REQUIRE(!C.cb_elim[C.cols.cb_of[hub]]);                       // the hub has the most neighbours: it stays
    REQUIRE(C.F.parts.long_owner.size() == 1 && C.E.parts.long_owner.empty());
    printf("cgnr_schur_plan_check chain ok: %zu eliminated, %zu kept (%d columns), %zu pairs, %zu pair parts\n", C.E.cb.size(), C.F.cb.size(), C.reduced_cols,
           C.fp_e.size(), C.fp_parts.owner.size());
  }
  // bundle adjustment
  {
    const int cams = 5, points = 150;
    std::vector<int> sizes(cams, 9);
    sizes.insert(sizes.end(), points, 3);
    Builder B(sizes);
    for (int q = 0; q + 1 < points; ++q) for (int k = 0; k < 3; ++k) B.add(SK_FUNCTOR_SNAVELY_REPROJECTION, 2, 2, (q + k) % cams, cams + q);
    for (int rep = 0; rep < 20; ++rep) for (int c = 0; c < cams; ++c) B.add(SK_FUNCTOR_SNAVELY_REPROJECTION, 2, 2, c, cams + points - 1);   // 100 slots: two parts
    B.add(SK_FUNCTOR_SNAVELY_REPROJECTION, 2, 2, 2, cams + 7);   // a repeated observation
    B.p.block_constant[0] = 1;
    REQUIRE(cgnr_refusal(B.p, 1, false).empty());
    CgnrPlan C, plain;
    std::string why;
    REQUIRE(cgnr_plan_build(B.p, &plain, &why) == SK_OK && cgnr_plan_build(B.p, &C, &why, true) == SK_OK);
    const int rc = check(B.p, C, plain);
    if (rc) return rc;
    REQUIRE((int)C.E.cb.size() == points && (int)C.F.cb.size() == cams - 1 && C.reduced_cols == 9 * (cams - 1));
    REQUIRE(C.E.parts.long_owner.size() == 1 && C.E.parts.long_owner[0] == points - 1);
    REQUIRE((int)C.fp_parts.long_owner.size() == cams - 1);        // a camera sees about 90 points: its pair list has two parts
    // the repeated observation: the pair (camera 2, point 7) has two terms
    int two = 0;
    for (size_t q = 0; q < C.fp_e.size(); ++q) if (C.fp_slot_begin[q + 1] - C.fp_slot_begin[q] == 2 && C.cols.cb_block[C.fp_e[q]] == cams + 7) ++two;
    REQUIRE(two == 1);
    printf("cgnr_schur_plan_check bundle adjustment ok: %zu eliminated, %zu kept, %zu pairs, %zu long e-blocks\n", C.E.cb.size(), C.F.cb.size(), C.fp_e.size(),
           C.E.parts.long_owner.size());
  }
  // no F at all: three unrelated blocks
  {
    Builder B(std::vector<int>(4, 2));
    B.add(SK_FUNCTOR_BINARY_VECTOR3_COST, 3, 1, 0, 1);
    B.p.block_constant[1] = 1;
    B.add(SK_FUNCTOR_BINARY_VECTOR3_COST, 3, 1, 2, 1);
    B.add(SK_FUNCTOR_BINARY_VECTOR3_COST, 3, 1, 1, 3);
    CgnrPlan C, plain;
    std::string why;
    REQUIRE(cgnr_plan_build(B.p, &plain, &why) == SK_OK && cgnr_plan_build(B.p, &C, &why, true) == SK_OK);
    const int rc = check(B.p, C, plain);
    if (rc) return rc;
    REQUIRE(C.F.cb.empty() && C.E.cb.size() == 3 && C.reduced_cols == 0 && C.fp_e.empty() && C.fp_parts.owner.empty());
    printf("cgnr_schur_plan_check empty F ok\n");
  }
  return 0;
}
