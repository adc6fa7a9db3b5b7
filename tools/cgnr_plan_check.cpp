// Stand-alone check of the host-only CGNR plan (skeres_amd/csrc/cgnr_plan.cpp): builds the plan for the structure of the `chain`
// case of tests/cgnr_cases.py — 2100 blocks of size 2 joined by three-row residual blocks between neighbours, every fifth
// listed in reverse column order, a hub block in 320 more of them, two constant blocks — and verifies what the kernels rely on.
// Meant to be compiled with the host compiler under -fsanitize=address,undefined (no device code, no HIP):
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       tools/cgnr_plan_check.cpp skeres_amd/csrc/cgnr_plan.cpp skeres_amd/csrc/jacobian_plan.cpp skeres_amd/csrc/evaluate_plan.cpp -o cgnr_plan_check && ./cgnr_plan_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../skeres_amd/csrc/cgnr_plan.hpp"

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "cgnr_plan_check: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

int main() {
  using namespace sk;
  const int nblocks = 2100, hub = 7, hub_blocks = 320;
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
  for (int k = 0; k < hub_blocks; ++k) { const int j = 20 + 6 * k; if (k % 2 == 0) add(hub, j); else add(j, hub); }
  p.block_constant[block(100)] = 1; p.block_constant[block(101)] = 1;

  REQUIRE(cgnr_refusal(p, 1, false).empty());
  REQUIRE(!cgnr_refusal(p, 2, false).empty() && !cgnr_refusal(p, 1, true).empty());
  CgnrPlan C;
  std::string why;
  REQUIRE(cgnr_plan_build(p, &C, &why) == SK_OK);
  const EvaluatePlan& E = C.eval;
  const int ncb = (int)C.cols.cb_col.size(), ns = (int)E.slot_block.size(), nparts = (int)C.parts.owner.size();
  REQUIRE(C.cols.num_ambient == 2 * nblocks && C.cols.num_cols == 2 * (nblocks - 2) && ncb == nblocks - 2);
  REQUIRE(E.num_rows == 3 * (nblocks - 1 + hub_blocks) && (int)C.row_block.size() == E.num_rows);
  // every stored slot once in exactly one column block's list, in ascending order; the values stay inside the array
  std::vector<int> seen(ns, 0);
  long long stored = 0;
  for (int c = 0; c < ncb; ++c) {
    REQUIRE(C.cols.cb_size[c] == 2 && C.cols.cb_col[c] == 2 * c && C.cb_moff[c + 1] - C.cb_moff[c] == 4);
    for (int k = C.cb_begin[c]; k < C.cb_begin[c + 1]; ++k) {
      const int s = C.cb_slots[k];
      REQUIRE(s >= 0 && s < ns && !seen[s]++ && C.slot_col[s] == C.cols.cb_col[c] && C.slot_size[s] == C.cols.cb_size[c]);
      REQUIRE(k == C.cb_begin[c] || C.cb_slots[k - 1] < s);
      const int i = E.slot_owner[s], nres = E.row_off[i + 1] - E.row_off[i], width = (E.val_off[i + 1] - E.val_off[i]) / nres;
      REQUIRE(E.slot_pos[s] >= 0 && E.slot_pos[s] + C.slot_size[s] <= width && E.val_off[i + 1] <= E.num_nonzeros);
      stored += (long long)nres * C.slot_size[s];
    }
  }
  REQUIRE(stored == E.num_nonzeros);
  for (int s = 0; s < ns; ++s) REQUIRE(seen[s] == (E.slot_pos[s] >= 0 ? 1 : 0) && (E.slot_pos[s] >= 0) == (C.slot_col[s] >= 0));
  // the parts tile every list in order, kCgnrPartSlots at a time; the long blocks' partial sums are numbered consecutively
  int part = 0, partial = 0, nlong = 0;
  for (int c = 0; c < ncb; ++c) {
    const int begin = C.cb_begin[c], end = C.cb_begin[c + 1], first = part;
    int at = begin;
    do {
      REQUIRE(part < nparts && C.parts.owner[part] == c && C.parts.begin[part] == at);
      REQUIRE(C.parts.end[part] == (at + kCgnrPartSlots < end ? at + kCgnrPartSlots : end));
      at = C.parts.end[part++];
    } while (at < end);
    if (part - first == 1) { REQUIRE(C.parts.out[first] == -1); continue; }
    REQUIRE(C.parts.long_owner[nlong] == c && C.parts.long_begin[nlong] == partial);
    for (int k = first; k < part; ++k) REQUIRE(C.parts.out[k] == partial++);
    REQUIRE(C.parts.long_begin[++nlong] == partial);
  }
  REQUIRE(part == nparts && partial == C.parts.num_partials && nlong == (int)C.parts.long_owner.size());
  REQUIRE(nlong == 1 && C.parts.num_partials == (hub_blocks + 2 + kCgnrPartSlots - 1) / kCgnrPartSlots);   // the hub: 320 + its two neighbours
  REQUIRE(C.blk_stage_cost.size() == E.blk_stage.size() && C.group_stage_cost.size() == E.groups.size());
  printf("cgnr_plan_check ok: %d column blocks, %d parts, %d long, %lld stored entries\n", ncb, nparts, nlong, E.num_nonzeros);

  // cut_parts by itself: owners with lists of 0, 1, 64, 65 and 129 entries in one call
  const int lengths[5] = {0, 1, 64, 65, 129}, want_parts[5] = {1, 1, 1, 2, 3};
  std::vector<int> begin_of(1, 0);
  for (int len : lengths) begin_of.push_back(begin_of.back() + len);
  PartList L;
  cut_parts(begin_of, &L);
  const size_t total = 1 + 1 + 1 + 2 + 3;
  REQUIRE(L.owner.size() == total && L.begin.size() == total && L.end.size() == total && L.out.size() == total);
  int k = 0, partials = 0, longs = 0;
  REQUIRE(L.long_begin.size() >= 1 && L.long_begin[0] == 0);
  for (int q = 0; q < 5; ++q) {
    int at = begin_of[q];
    for (int j = 0; j < want_parts[q]; ++j, ++k) {
      REQUIRE(L.owner[k] == q && L.begin[k] == at && L.end[k] == std::min(at + kCgnrPartSlots, begin_of[q + 1]) && L.end[k] >= L.begin[k]);
      REQUIRE(L.out[k] == (want_parts[q] == 1 ? -1 : partials));   // -1 exactly for the owners of one part
      if (want_parts[q] > 1) ++partials;
      at = L.end[k];
    }
    REQUIRE(at == begin_of[q + 1]);
    if (want_parts[q] == 1) continue;
    REQUIRE(longs < (int)L.long_owner.size() && L.long_owner[longs] == q);
    REQUIRE(L.long_begin[longs] < L.long_begin[longs + 1] && L.long_begin[longs + 1] == partials);   // monotone
    ++longs;
  }
  REQUIRE(L.begin[0] == 0 && L.end[0] == 0);   // the empty owner: one empty part
  REQUIRE(longs == 2 && (int)L.long_owner.size() == longs && (int)L.long_begin.size() == longs + 1 && L.long_begin.back() == L.num_partials && L.num_partials == 5);
  printf("cgnr_plan_check cut_parts ok: %zu parts, %d long, %d partial sums\n", total, longs, L.num_partials);
  return 0;
}
