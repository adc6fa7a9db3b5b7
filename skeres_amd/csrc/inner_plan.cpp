// Host plan of the inner iterations — see inner_plan.hpp.  No HIP in this file.
#include "inner_plan.hpp"

#include <algorithm>
#include <cstdio>

namespace sk {

std::string inner_refusal(int linear_solver_type, const char* name) {
  if (linear_solver_type == SK_CGNR) return "";
  return std::string("use_inner_iterations is implemented for CGNR (not supported under ") + name + ")";
}

namespace {

// The stored column blocks of residual block i, in slot order (a block named twice appears twice)
void stored_blocks(const CgnrPlan& C, int i, std::vector<int>* out) {
  const EvaluatePlan& E = C.eval;
  out->clear();
  for (int s = E.slot_begin[i]; s < E.slot_begin[i + 1]; ++s) if (E.slot_pos[s] >= 0) out->push_back(C.cols.cb_of[E.slot_block[s]]);
}

// Group k of the automatic ordering: the greedy independent set of the ungrouped blocks, neighbours counted among them alone
void automatic_groups(const CgnrPlan& C, std::vector<int>* group_of_cb) {
  const int ncb = (int)C.cols.cb_col.size(), nb = (int)C.eval.blocks.size();
  std::vector<int>& G = *group_of_cb;
  G.assign(ncb, -1);
  std::vector<int> stored, local(ncb), members;
  for (int k = 0;; ++k) {
    members.clear();
    for (int c = 0; c < ncb; ++c) { local[c] = -1; if (G[c] < 0) { local[c] = (int)members.size(); members.push_back(c); } }
    const int nm = (int)members.size();
    if (nm == 0) return;
    std::vector<long long> edges;
    for (int i = 0; i < nb; ++i) {
      stored_blocks(C, i, &stored);
      for (int a : stored) for (int b : stored) if (a != b && local[a] >= 0 && local[b] >= 0) edges.push_back((long long)local[a] * nm + local[b]);
    }
    std::sort(edges.begin(), edges.end());
    edges.erase(std::unique(edges.begin(), edges.end()), edges.end());
    std::vector<int> nb_begin(nm + 1, 0), nbr(edges.size()), in_set;
    for (size_t e = 0; e < edges.size(); ++e) { ++nb_begin[edges[e] / nm + 1]; nbr[e] = (int)(edges[e] % nm); }
    for (int c = 0; c < nm; ++c) nb_begin[c + 1] += nb_begin[c];
    greedy_independent_set(nb_begin, nbr, &in_set);
    for (int c = 0; c < nm; ++c) if (in_set[c]) G[members[c]] = k;  // (the first block visited always joins: the loop ends)
  }
}

}  // namespace

int inner_plan_build(const Problem& p, const CgnrPlan& C, const std::vector<double*>& blocks, const std::vector<int>& groups, InnerPlan* plan, std::string* why) {
  InnerPlan& P = *plan;
  P = InnerPlan();
  const EvaluatePlan& E = C.eval;
  const TangentColumns& T = C.cols;
  const int ncb = (int)T.cb_col.size(), nb = (int)E.blocks.size();
  char buf[256];
  if (blocks.empty()) {
    automatic_groups(C, &P.group_of_cb);
  } else {
    if (blocks.size() != groups.size()) { *why = "inner_iteration_ordering: one group id per block"; return SK_ERR_INVALID_ARGUMENT; }
    P.group_of_cb.assign(ncb, -1);
    std::vector<int> ids;
    for (size_t k = 0; k < blocks.size(); ++k) {
      const auto it = p.block_of.find(blocks[k]);
      if (it == p.block_of.end()) {
        snprintf(buf, sizeof(buf), "inner_iteration_ordering: entry %d is not a parameter block of the problem", (int)k);
        *why = buf; return SK_ERR_INVALID_ARGUMENT;
      }
      if (groups[k] < 0) {
        snprintf(buf, sizeof(buf), "inner_iteration_ordering: entry %d (parameter block %d) has the negative group id %d", (int)k, it->second, groups[k]);
        *why = buf; return SK_ERR_INVALID_ARGUMENT;
      }
      const int c = T.cb_of[it->second];
      if (c < 0) continue;  // constant, or no tangent columns: ignored
      P.group_of_cb[c] = groups[k];
      ids.push_back(groups[k]);
    }
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    for (int c = 0; c < ncb; ++c)
      if (P.group_of_cb[c] >= 0) P.group_of_cb[c] = (int)(std::lower_bound(ids.begin(), ids.end(), P.group_of_cb[c]) - ids.begin());
  }
  // independence: no residual block names two different blocks of one group
  std::vector<int> stored;
  for (int i = 0; i < nb; ++i) {
    stored_blocks(C, i, &stored);
    for (size_t a = 0; a < stored.size(); ++a)
      for (size_t b = a + 1; b < stored.size(); ++b) {
        const int ca = stored[a], cb = stored[b];
        if (ca == cb || P.group_of_cb[ca] < 0 || P.group_of_cb[ca] != P.group_of_cb[cb]) continue;
        snprintf(buf, sizeof(buf), "inner_iteration_ordering: group %d is not an independent set: residual block %d names its parameter blocks %d and %d",
                 P.group_of_cb[ca], i, T.cb_block[ca], T.cb_block[cb]);
        *why = buf; return SK_ERR_INVALID_ARGUMENT;
      }
  }
  int ngroups = 0;
  for (int c = 0; c < ncb; ++c) ngroups = std::max(ngroups, P.group_of_cb[c] + 1);
  P.groups.resize(ngroups);
  for (int c = 0; c < ncb; ++c) if (P.group_of_cb[c] >= 0) P.groups[P.group_of_cb[c]].blocks.cb.push_back(c);
  for (InnerGroup& G : P.groups) {
    CgnrColumnSubset& S = G.blocks;
    S.cb_begin.push_back(0);
    for (int c : S.cb) {
      G.pb.push_back(T.cb_block[c]);
      S.cb_col.push_back(T.cb_col[c]); S.cb_size.push_back(T.cb_size[c]); S.cb_moff.push_back(C.cb_moff[c]);
      for (int k = C.cb_begin[c]; k < C.cb_begin[c + 1]; ++k) {
        const int slot = C.cb_slots[k], i = E.slot_owner[slot];
        const bool again = k > C.cb_begin[c] && E.slot_owner[C.cb_slots[k - 1]] == i;  // (slots ascend with the rows: a block's slots of one residual block are neighbours)
        S.cb_slots.push_back(slot);
        G.cost_rb.push_back(again ? -1 : i);
      }
      S.cb_begin.push_back((int)S.cb_slots.size());
    }
    cut_parts(S.cb_begin, &S.parts);
    P.max_group_blocks = std::max(P.max_group_blocks, (int)S.cb.size());
    P.max_partials = std::max(P.max_partials, S.parts.num_partials);
  }
  return SK_OK;
}

}  // namespace sk
