// Host plan of the CGNR solver — see cgnr_plan.hpp.  No HIP in this file.
#include "cgnr_plan.hpp"

#include <algorithm>
#include <cstdio>

namespace sk {

std::string cgnr_refusal(const Problem& p, int world, bool dogleg) {
  char buf[256];
  if (dogleg) return "CGNR with DOGLEG is not supported (LEVENBERG_MARQUARDT is: the inexact step has no Gauss-Newton / Cauchy pair)";
  if (world > 1) {
    snprintf(buf, sizeof(buf), "CGNR is implemented for one device (not supported in a world of %d ranks)", world);
    return buf;
  }
  if (p.has_bounds()) return "parameter bounds under CGNR are not supported (DENSE_SCHUR and DENSE_QR / DENSE_NORMAL_CHOLESKY take them)";
  for (size_t b = 0; b < p.rb_functor.size(); ++b) {
    if (p.rb_functor[b] == SK_FUNCTOR_SYNTH_TANH_ROW) return "CGNR works on a block-sparse Jacobian: dense-row problems are not supported (DENSE_NORMAL_CHOLESKY takes them)";
    if (p.rb_functor[b] == SK_FUNCTOR_HOST_CALLBACK) {
      snprintf(buf, sizeof(buf), "CGNR with host-evaluated (director) residual blocks is not supported (residual block %d; DENSE_QR takes them)", (int)b);
      return buf;
    }
  }
  return block_size_refusal(p, "CGNR", kCgnrMaxBlock, /*constants_too*/ false);
}

namespace {

// The column blocks `members` (ascending) of C as a list of their own
void column_subset_build(const CgnrPlan& C, const std::vector<int>& members, CgnrColumnSubset* subset) {
  CgnrColumnSubset& S = *subset;
  S = CgnrColumnSubset();
  S.cb = members;
  S.cb_begin.push_back(0);
  for (int c : members) {
    S.cb_col.push_back(C.cols.cb_col[c]); S.cb_size.push_back(C.cols.cb_size[c]); S.cb_moff.push_back(C.cb_moff[c]);
    S.cb_slots.insert(S.cb_slots.end(), C.cb_slots.begin() + C.cb_begin[c], C.cb_slots.begin() + C.cb_begin[c + 1]);
    S.cb_begin.push_back((int)S.cb_slots.size());
  }
  cut_parts(S.cb_begin, &S.parts);
}

// E, F and the pair lists of the block diagonal of S (cgnr_plan.hpp); the columns and slot lists of C are built
void schur_elimination_build(CgnrPlan& C) {
  const EvaluatePlan& E = C.eval;
  const TangentColumns& T = C.cols;
  const int ncb = (int)T.cb_col.size(), nb = (int)E.blocks.size();
  // every (column block, column block) that a residual block names, both ways, each once: the distinct neighbours
  std::vector<long long> edges;
  std::vector<int> stored;
  for (int i = 0; i < nb; ++i) {
    stored.clear();
    for (int s = E.slot_begin[i]; s < E.slot_begin[i + 1]; ++s) if (E.slot_pos[s] >= 0) stored.push_back(T.cb_of[E.slot_block[s]]);
    for (int a : stored) for (int b : stored) if (a != b) edges.push_back((long long)a * ncb + b);
  }
  std::sort(edges.begin(), edges.end());
  edges.erase(std::unique(edges.begin(), edges.end()), edges.end());
  std::vector<int> nb_begin(ncb + 1, 0), nbr(edges.size());
  for (size_t k = 0; k < edges.size(); ++k) { ++nb_begin[edges[k] / ncb + 1]; nbr[k] = (int)(edges[k] % ncb); }
  for (int c = 0; c < ncb; ++c) nb_begin[c + 1] += nb_begin[c];
  greedy_independent_set(nb_begin, nbr, &C.cb_elim);

  std::vector<int> in_f, in_e, f_of(ncb, -1);
  for (int c = 0; c < ncb; ++c) {
    if (C.cb_elim[c]) { in_e.push_back(c); continue; }
    f_of[c] = (int)in_f.size(); in_f.push_back(c); C.reduced_cols += T.cb_size[c];
  }
  column_subset_build(C, in_f, &C.F);
  column_subset_build(C, in_e, &C.E);
  C.slot_size_f = C.slot_size;
  for (size_t s = 0; s < C.slot_size_f.size(); ++s) if (E.slot_pos[s] >= 0 && C.cb_elim[T.cb_of[E.slot_block[s]]]) C.slot_size_f[s] = 0;

  // the terms of the pairs: per residual block every (slot of an F block, slot of an e-block); sorted by (g, e), rows kept in order
  struct Term { long long key; int sg, se; };
  std::vector<Term> terms;
  for (int i = 0; i < nb; ++i)
    for (int sg = E.slot_begin[i]; sg < E.slot_begin[i + 1]; ++sg) {
      if (E.slot_pos[sg] < 0 || C.cb_elim[T.cb_of[E.slot_block[sg]]]) continue;
      for (int se = E.slot_begin[i]; se < E.slot_begin[i + 1]; ++se) {
        if (E.slot_pos[se] < 0 || !C.cb_elim[T.cb_of[E.slot_block[se]]]) continue;
        terms.push_back(Term{(long long)f_of[T.cb_of[E.slot_block[sg]]] * ncb + T.cb_of[E.slot_block[se]], sg, se});
      }
    }
  std::stable_sort(terms.begin(), terms.end(), [](const Term& a, const Term& b) { return a.key < b.key; });
  C.fp_begin.assign(in_f.size() + 1, 0);
  for (size_t t = 0; t < terms.size(); ++t) {
    if (t == 0 || terms[t].key != terms[t - 1].key) {
      ++C.fp_begin[terms[t].key / ncb + 1];
      C.fp_e.push_back((int)(terms[t].key % ncb)); C.fp_slot_begin.push_back((int)t);
    }
    C.fp_slot_g.push_back(terms[t].sg); C.fp_slot_e.push_back(terms[t].se);
  }
  C.fp_slot_begin.push_back((int)terms.size());
  for (size_t f = 0; f < in_f.size(); ++f) C.fp_begin[f + 1] += C.fp_begin[f];
  cut_parts(C.fp_begin, &C.fp_parts);
}

}  // namespace

int cgnr_plan_build(const Problem& p, CgnrPlan* plan, std::string* why, bool schur_elimination) {
  CgnrPlan& C = *plan;
  C = CgnrPlan();
  int rc = evaluate_plan_build(p, nullptr, false, false, true, &C.eval, why);
  if (rc != SK_OK) return rc;
  const EvaluatePlan& E = C.eval;
  evaluate_plan_staging(E, /*jacobian*/ false, &C.group_stage_cost, &C.blk_stage_cost);  // of a residual-only evaluation: the same groups, num_residuals planes each
  const int nb = (int)E.blocks.size(), ns = (int)E.slot_block.size();
  tangent_columns_build(p, E, ConstantTangent::kZero, &C.cols);
  const TangentColumns& T = C.cols;
  const int ncb = (int)T.cb_col.size();
  C.cb_moff.assign(ncb + 1, 0);
  for (int c = 0; c < ncb; ++c) C.cb_moff[c + 1] = C.cb_moff[c] + T.cb_size[c] * T.cb_size[c];

  C.slot_col.assign(ns, -1); C.slot_size.assign(ns, 0);
  C.cb_begin.assign(ncb + 1, 0);
  for (int s = 0; s < ns; ++s) {
    if (E.slot_pos[s] < 0) continue;
    const int b = E.slot_block[s];
    C.slot_col[s] = T.pb_local_off[b]; C.slot_size[s] = T.pb_local_size[b];
    ++C.cb_begin[T.cb_of[b] + 1];
  }
  for (int c = 0; c < ncb; ++c) C.cb_begin[c + 1] += C.cb_begin[c];
  C.cb_slots.resize(C.cb_begin[ncb]);
  {
    std::vector<int> fill(C.cb_begin.begin(), C.cb_begin.end() - 1);
    for (int s = 0; s < ns; ++s) if (E.slot_pos[s] >= 0) C.cb_slots[fill[T.cb_of[E.slot_block[s]]]++] = s;  // slots ascend with the rows
  }

  C.row_block.resize((size_t)E.num_rows);
  for (int i = 0; i < nb; ++i) for (int r = E.row_off[i]; r < E.row_off[i + 1]; ++r) C.row_block[r] = i;

  cut_parts(C.cb_begin, &C.parts);  // (a block without slots — nothing observes it — has one empty part)
  if (schur_elimination) schur_elimination_build(C);
  return SK_OK;
}

}  // namespace sk
