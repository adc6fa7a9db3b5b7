// Stand-alone check of the host-only plan of the inner iterations (skeres_amd/csrc/inner_plan.cpp): builds the plan for the
// structure of the `chain` case of tests/inner_cases.py — 145 blocks of size 2 joined by three-row residual blocks between
// neighbours, every fifth listed in reverse column order, a hub block in 63 more of them, two constant blocks — and verifies what
// the kernels rely on: the groups are independent, they cover every moving block once, and the parts tile the slot lists.
// Meant to be compiled with the host compiler under -fsanitize=address,undefined (no device code, no HIP):
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include tools/inner_plan_check.cpp \
//       skeres_amd/csrc/inner_plan.cpp skeres_amd/csrc/cgnr_plan.cpp skeres_amd/csrc/jacobian_plan.cpp skeres_amd/csrc/evaluate_plan.cpp \
//       -o inner_plan_check && ./inner_plan_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../skeres_amd/csrc/inner_plan.hpp"

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "inner_plan_check: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

using namespace sk;

// independence, cover (every block of `want` in exactly one group, nothing else) and the tiling of one plan
static int check(const CgnrPlan& C, const InnerPlan& P, const std::vector<int>& want) {
  const EvaluatePlan& E = C.eval;
  const int ncb = (int)C.cols.cb_col.size(), nb = (int)E.blocks.size();
  REQUIRE((int)P.group_of_cb.size() == ncb && (int)want.size() == ncb);
  std::vector<int> seen(ncb, 0);
  int max_blocks = 0, max_partials = 0;
  for (size_t g = 0; g < P.groups.size(); ++g) {
    const InnerGroup& G = P.groups[g];
    const CgnrColumnSubset& S = G.blocks;
    const int n = (int)S.cb.size();
    REQUIRE(n > 0 && (int)G.pb.size() == n && (int)S.cb_col.size() == n && (int)S.cb_size.size() == n && (int)S.cb_moff.size() == n && (int)S.cb_begin.size() == n + 1);
    REQUIRE(G.cost_rb.size() == S.cb_slots.size() && S.cb_begin[0] == 0 && S.cb_begin[n] == (int)S.cb_slots.size());
    int part = 0, partial = 0, nlong = 0;
    const int nparts = (int)S.parts.owner.size();
    for (int e = 0; e < n; ++e) {
      const int c = S.cb[e];
      REQUIRE(c >= 0 && c < ncb && (e == 0 || S.cb[e - 1] < c) && !seen[c]++ && P.group_of_cb[c] == (int)g);
      REQUIRE(G.pb[e] == C.cols.cb_block[c] && S.cb_col[e] == C.cols.cb_col[c] && S.cb_size[e] == C.cols.cb_size[c] && S.cb_moff[e] == C.cb_moff[c]);
      // the block's slot list is the CGNR plan's; a residual block's cost term is named once
      REQUIRE(S.cb_begin[e + 1] - S.cb_begin[e] == C.cb_begin[c + 1] - C.cb_begin[c]);
      std::vector<int> named;
      for (int k = S.cb_begin[e]; k < S.cb_begin[e + 1]; ++k) {
        const int slot = S.cb_slots[k];
        REQUIRE(slot == C.cb_slots[C.cb_begin[c] + (k - S.cb_begin[e])] && C.slot_col[slot] == S.cb_col[e]);
        REQUIRE(G.cost_rb[k] == -1 || G.cost_rb[k] == E.slot_owner[slot]);
        if (G.cost_rb[k] >= 0) named.push_back(G.cost_rb[k]);
        else REQUIRE(std::find(named.begin(), named.end(), E.slot_owner[slot]) != named.end());
      }
      for (size_t a = 1; a < named.size(); ++a) REQUIRE(named[a - 1] < named[a]);
      // the parts tile the list in order, kCgnrPartSlots at a time
      const int begin = S.cb_begin[e], end = S.cb_begin[e + 1], first = part;
      int at = begin;
      do {
        REQUIRE(part < nparts && S.parts.owner[part] == e && S.parts.begin[part] == at);
        REQUIRE(S.parts.end[part] == (at + kCgnrPartSlots < end ? at + kCgnrPartSlots : end));
        at = S.parts.end[part++];
      } while (at < end);
      if (part - first == 1) { REQUIRE(S.parts.out[first] == -1); continue; }
      REQUIRE(S.parts.long_owner[nlong] == e && S.parts.long_begin[nlong] == partial);
      for (int k = first; k < part; ++k) REQUIRE(S.parts.out[k] == partial++);
      REQUIRE(S.parts.long_begin[++nlong] == partial);
    }
    REQUIRE(part == nparts && partial == S.parts.num_partials && nlong == (int)S.parts.long_owner.size());
    max_blocks = std::max(max_blocks, n); max_partials = std::max(max_partials, partial);
  }
  REQUIRE(P.max_group_blocks == max_blocks && P.max_partials == max_partials);
  for (int c = 0; c < ncb; ++c) REQUIRE(seen[c] == want[c] && (P.group_of_cb[c] >= 0) == (want[c] == 1));
  // independence: no residual block names two different blocks of one group
  for (int i = 0; i < nb; ++i)
    for (int a = E.slot_begin[i]; a < E.slot_begin[i + 1]; ++a)
      for (int b = a + 1; b < E.slot_begin[i + 1]; ++b) {
        if (E.slot_pos[a] < 0 || E.slot_pos[b] < 0) continue;
        const int ca = C.cols.cb_of[E.slot_block[a]], cb = C.cols.cb_of[E.slot_block[b]];
        REQUIRE(ca == cb || P.group_of_cb[ca] < 0 || P.group_of_cb[ca] != P.group_of_cb[cb]);
      }
  return 0;
}

int main() {
  const int nblocks = 145, hub = 7, hub_blocks = 63;
  std::vector<double> x(2 * nblocks, 1.0);
  Problem p;
  auto block = [&](int b) {
    double* ptr = &x[2 * b];
    auto it = p.block_of.find(ptr);
    if (it != p.block_of.end()) return it->second;
    const int id = (int)p.block_ptr.size();
    p.block_of.emplace(ptr, id); p.block_ptr.push_back(ptr); p.block_size.push_back(2);
    p.block_param.push_back(-1); p.block_constant.push_back(0);
    return id;
  };
  auto add = [&](int a, int b) {
    p.rb_functor.push_back(SK_FUNCTOR_BINARY_VECTOR3_COST); p.rb_num_residuals.push_back(3); p.rb_const_off.push_back(p.consts.size());
    p.consts.push_back(0.5); p.rb_cost.push_back(nullptr); p.rb_loss.push_back(-1);
    p.rb_pidx.push_back(block(a)); p.rb_pidx.push_back(block(b)); p.rb_pidx_off.push_back(p.rb_pidx.size());
    p.num_residuals += 3;
  };
  for (int i = 0; i + 1 < nblocks; ++i) { if (i % 5 == 0) add(i + 1, i); else add(i, i + 1); }
  for (int k = 0; k < hub_blocks; ++k) { const int j = 20 + 2 * k; if (k % 2 == 0) add(hub, j); else add(j, hub); }
  p.block_constant[block(100)] = 1; p.block_constant[block(101)] = 1;

  REQUIRE(inner_refusal(SK_CGNR, "CGNR").empty());
  REQUIRE(inner_refusal(SK_DENSE_SCHUR, "DENSE_SCHUR").find("DENSE_SCHUR") != std::string::npos);
  CgnrPlan C;
  std::string why;
  REQUIRE(cgnr_plan_build(p, &C, &why) == SK_OK);
  const int ncb = (int)C.cols.cb_col.size();
  REQUIRE(ncb == nblocks - 2);

  // automatic: every moving block in one group; a path needs two groups, the hub one more
  InnerPlan A;
  REQUIRE(inner_plan_build(p, C, {}, {}, &A, &why) == SK_OK);
  if (check(C, A, std::vector<int>(ncb, 1))) return 1;
  REQUIRE(A.groups.size() >= 3);
  const int hub_cb = C.cols.cb_of[block(hub)];
  REQUIRE(A.group_of_cb[hub_cb] >= 2);
  int hub_long = 0;
  for (const InnerGroup& G : A.groups) for (int e : G.blocks.parts.long_owner) hub_long += G.blocks.cb[e] == hub_cb;
  REQUIRE(hub_long == 1 && A.max_partials == (hub_blocks + 2 + kCgnrPartSlots - 1) / kCgnrPartSlots);
  printf("inner_plan_check ok: %d column blocks in %d groups, the hub in group %d with %d parts\n", ncb, (int)A.groups.size(), A.group_of_cb[hub_cb], A.max_partials);

  // the caller's: the even blocks as group 7 and two odd ones as group 2 (compressed to 1 and 0), a constant block ignored
  std::vector<double*> blocks;
  std::vector<int> groups, want(ncb, 0);
  for (int b = 0; b < nblocks; b += 2) { blocks.push_back(&x[2 * b]); groups.push_back(7); if (C.cols.cb_of[block(b)] >= 0) want[C.cols.cb_of[block(b)]] = 1; }
  for (int b : {31, 55}) { blocks.push_back(&x[2 * b]); groups.push_back(2); want[C.cols.cb_of[block(b)]] = 1; }
  InnerPlan U;
  REQUIRE(inner_plan_build(p, C, blocks, groups, &U, &why) == SK_OK);
  if (check(C, U, want)) return 1;
  REQUIRE(U.groups.size() == 2 && U.groups[0].blocks.cb.size() == 2 && U.group_of_cb[C.cols.cb_of[block(31)]] == 0 && U.group_of_cb[C.cols.cb_of[block(0)]] == 1);
  REQUIRE(C.cols.cb_of[block(100)] < 0);
  // refused: two neighbours in one group (the message names both), an unknown pointer, a negative group
  blocks.push_back(&x[2 * 1]); groups.push_back(7);
  REQUIRE(inner_plan_build(p, C, blocks, groups, &U, &why) == SK_ERR_INVALID_ARGUMENT);
  REQUIRE(why.find("not an independent set") != std::string::npos && why.find(std::to_string(block(1))) != std::string::npos);
  double outside = 0.0;
  blocks.back() = &outside;
  REQUIRE(inner_plan_build(p, C, blocks, groups, &U, &why) == SK_ERR_INVALID_ARGUMENT && why.find("not a parameter block") != std::string::npos);
  blocks.back() = &x[2 * 33]; groups.back() = -1;
  REQUIRE(inner_plan_build(p, C, blocks, groups, &U, &why) == SK_ERR_INVALID_ARGUMENT && why.find("negative") != std::string::npos);
  printf("inner_plan_check ordering ok: 2 groups of the caller's, 3 refusals\n");
  return 0;
}
