// Host plan of sk_covariance_compute — see covariance_plan.hpp.  No HIP in this file.
#include "covariance_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <map>

namespace sk {

std::string covariance_refusal(const Problem& p, bool schur) {
  char buf[320];
  for (size_t b = 0; b < p.rb_functor.size(); ++b)
    if (p.rb_functor[b] == SK_FUNCTOR_SYNTH_TANH_ROW)
      return "Covariance works on a block-sparse Jacobian: dense-row problems (sk_problem_add_dense_rows) are not supported";
  const std::string too_large = block_size_refusal(p, "Covariance", kCovarianceMaxBlock, /*constants_too*/ true);
  if (!too_large.empty()) return too_large;
  long long cols = 0;
  for (size_t b = 0; b < p.block_size.size(); ++b) {
    if (b < p.block_constant.size() && p.block_constant[b]) continue;
    const int pz = b < p.block_param.size() ? p.block_param[b] : -1;
    cols += pz >= 0 ? p.params[pz].local_size : p.block_size[b];
  }
  if (!schur && cols > kCovarianceMaxColumns) {
    snprintf(buf, sizeof(buf),
             "Covariance factors the dense normal matrix of the whole problem and takes up to %d columns (this problem has %lld: not supported); the "
             "bundle-adjustment route through the reduced camera system is not built into the dense route: see sk_covariance_options_set_schur_elimination",
             kCovarianceMaxColumns, cols);
    return buf;
  }
  return "";
}

namespace {
// E, the routing of the pairs, F(e) and the Schur terms (covariance_plan.hpp); the columns, pairs, terms and parts of C are built
int schur_plan_build(CovariancePlan& C, std::string* why) {
  const TangentColumns& T = C.cols;
  const int ncb = (int)T.cb_col.size(), npairs = (int)C.pair_i.size();
  C.schur = true;
  // neighbours: every off-diagonal pair names two
  std::vector<int> deg(ncb, 0), nb_begin(ncb + 1, 0);
  for (int q = 0; q < npairs; ++q) if (C.pair_i[q] != C.pair_j[q]) { ++deg[C.pair_i[q]]; ++deg[C.pair_j[q]]; }
  for (int c = 0; c < ncb; ++c) nb_begin[c + 1] = nb_begin[c] + deg[c];
  std::vector<int> nb(nb_begin[ncb]), fill(nb_begin.begin(), nb_begin.end() - 1);
  for (int q = 0; q < npairs; ++q) if (C.pair_i[q] != C.pair_j[q]) { nb[fill[C.pair_i[q]]++] = C.pair_j[q]; nb[fill[C.pair_j[q]]++] = C.pair_i[q]; }
  greedy_independent_set(nb_begin, nb, &C.cb_elim);  // (column blocks ascend with the parameter-block index)
  C.cb_red.assign(ncb, 0);
  long long red = 0;
  for (int c = 0; c < ncb; ++c) {
    if (C.cb_elim[c]) { C.cb_red[c] = (int)C.e_cb.size(); C.e_cb.push_back(c); }
    else { C.cb_red[c] = (int)red; red += T.cb_size[c]; }
  }
  C.num_elim = (int)C.e_cb.size();
  C.red_cols = (int)red;
  // tiles: V_e, L_e^-1, then the (f, e) pairs in pair order; F(e) in ascending column order of g
  C.num_tiles = 2 * C.num_elim;
  C.pair_tile.assign(npairs, -1); C.pair_flip.assign(npairs, 0);
  std::vector<int> fe_count(C.num_elim + 1, 0);
  for (int q = 0; q < npairs; ++q) {
    const int i = C.pair_i[q], j = C.pair_j[q];
    if (i == j) { if (C.cb_elim[i]) C.pair_tile[q] = C.cb_red[i]; continue; }
    if (!C.cb_elim[i] && !C.cb_elim[j]) continue;
    C.pair_flip[q] = C.cb_elim[i];
    C.pair_tile[q] = C.num_tiles++;
    ++fe_count[C.cb_red[C.cb_elim[i] ? i : j] + 1];
  }
  C.ew_begin.assign(C.num_elim + 1, 0);
  for (int e = 0; e < C.num_elim; ++e) C.ew_begin[e + 1] = C.ew_begin[e] + fe_count[e + 1];
  C.ew_tile.assign(C.ew_begin[C.num_elim], 0); C.ew_g.assign(C.ew_begin[C.num_elim], 0); C.ew_sel.assign(C.ew_begin[C.num_elim], -1);
  {
    std::vector<std::pair<int, int>> ge;  // (g, pair) per e, sorted by g below
    std::vector<int> at(C.ew_begin.begin(), C.ew_begin.end() - 1);
    for (int q = 0; q < npairs; ++q) {
      if (C.pair_tile[q] < 2 * C.num_elim) continue;
      const int e = C.cb_red[C.pair_flip[q] ? C.pair_i[q] : C.pair_j[q]], g = C.pair_flip[q] ? C.pair_j[q] : C.pair_i[q];
      C.ew_g[at[e]] = g; C.ew_tile[at[e]] = C.pair_tile[q]; ++at[e];
    }
    for (int e = 0; e < C.num_elim; ++e) {
      ge.clear();
      for (int k = C.ew_begin[e]; k < C.ew_begin[e + 1]; ++k) ge.emplace_back(C.ew_g[k], C.ew_tile[k]);
      std::sort(ge.begin(), ge.end());
      for (int k = C.ew_begin[e]; k < C.ew_begin[e + 1]; ++k) { C.ew_g[k] = ge[k - C.ew_begin[e]].first; C.ew_tile[k] = ge[k - C.ew_begin[e]].second; }
    }
  }
  // the Schur terms: counted first (the refusals need no memory), then listed e by e and sorted by pair (stable: ascending e inside a pair)
  C.schur_terms = 0;
  for (int e = 0; e < C.num_elim; ++e) { const long long k = C.ew_begin[e + 1] - C.ew_begin[e]; C.schur_terms += k * (k + 1) / 2; }
  char buf[320];
  if (C.red_cols > kCovarianceMaxColumns) {
    snprintf(buf, sizeof(buf), "Covariance with Schur elimination factors the dense reduced matrix and takes up to %d columns after the elimination (this problem keeps %d of %d: not supported)",
             kCovarianceMaxColumns, C.red_cols, T.num_cols);
    if (why) *why = buf;
    return SK_ERR_UNSUPPORTED;
  }
  if (C.schur_terms > 2147483647LL) {
    snprintf(buf, sizeof(buf), "Covariance with Schur elimination takes up to 2147483647 Schur terms (this problem has %lld: not supported)", C.schur_terms);
    if (why) *why = buf;
    return SK_ERR_UNSUPPORTED;
  }
  struct STerm { long long key; int a, b, ne; };
  std::vector<STerm> st;
  st.reserve((size_t)C.schur_terms);
  for (int e = 0; e < C.num_elim; ++e)
    for (int k = C.ew_begin[e]; k < C.ew_begin[e + 1]; ++k)
      for (int l = C.ew_begin[e]; l <= k; ++l)
        st.push_back(STerm{(long long)C.ew_g[k] * ncb + C.ew_g[l], C.ew_tile[k], C.ew_tile[l], T.cb_size[C.e_cb[e]]});
  std::stable_sort(st.begin(), st.end(), [](const STerm& a, const STerm& b) { return a.key < b.key; });
  C.st_a.reserve(st.size()); C.st_b.reserve(st.size()); C.st_ne.reserve(st.size());
  for (size_t t = 0; t < st.size(); ++t) {
    if (t == 0 || st[t].key != st[t - 1].key) { C.sp_i.push_back((int)(st[t].key / ncb)); C.sp_j.push_back((int)(st[t].key % ncb)); C.sp_begin.push_back((int)t); }
    C.st_a.push_back(st[t].a); C.st_b.push_back(st[t].b); C.st_ne.push_back(st[t].ne);
  }
  C.sp_begin.push_back((int)st.size());
  cut_parts(C.sp_begin, &C.schur_parts);
  return SK_OK;
}
}  // namespace

int covariance_plan_build(const Problem& p, const std::vector<std::pair<int, int>>& pairs, CovariancePlan* plan, std::string* why, bool schur) {
  CovariancePlan& C = *plan;
  C = CovariancePlan();
  const std::string refusal = covariance_refusal(p, schur);
  if (!refusal.empty()) { if (why) *why = refusal; return SK_ERR_UNSUPPORTED; }
  int rc = evaluate_plan_build(p, nullptr, false, false, true, &C.eval, why);
  if (rc != SK_OK) return rc;
  const EvaluatePlan& E = C.eval;
  const int num_pb = (int)p.block_ptr.size(), nb = (int)E.blocks.size();

  tangent_columns_build(p, E, ConstantTangent::kKeep, &C.cols);
  const TangentColumns& T = C.cols;
  const int ncb = (int)T.cb_col.size();

  // terms: per residual block every (slot of i, slot of j) with i >= j; a block that a residual block names twice has the two
  // cross terms of its diagonal pair in both orders (J_s^T J_t + J_t^T J_s)
  struct Term { long long key; int si, sj; };
  std::vector<Term> terms;
  std::vector<int> stored;
  for (int i = 0; i < nb; ++i) {
    stored.clear();
    for (int s = E.slot_begin[i]; s < E.slot_begin[i + 1]; ++s) if (E.slot_pos[s] >= 0) stored.push_back(s);
    for (int s : stored)
      for (int t : stored) {
        const int ci = T.cb_of[E.slot_block[s]], cj = T.cb_of[E.slot_block[t]];
        if (ci < cj) continue;
        terms.push_back(Term{(long long)ci * ncb + cj, s, t});
      }
  }
  std::stable_sort(terms.begin(), terms.end(), [](const Term& a, const Term& b) { return a.key < b.key; });  // (row order inside a pair is kept)
  C.term_si.reserve(terms.size()); C.term_sj.reserve(terms.size());
  for (size_t t = 0; t < terms.size(); ++t) {
    if (t == 0 || terms[t].key != terms[t - 1].key) {
      C.pair_i.push_back((int)(terms[t].key / ncb)); C.pair_j.push_back((int)(terms[t].key % ncb));
      C.pair_begin.push_back((int)t);
    }
    C.term_si.push_back(terms[t].si); C.term_sj.push_back(terms[t].sj);
  }
  C.pair_begin.push_back((int)terms.size());

  cut_parts(C.pair_begin, &C.pair_parts);
  if (schur) {
    rc = schur_plan_build(C, why);
    if (rc != SK_OK) return rc;
  }

  // the selection, in order of first appearance, and the requested pairs, each once.  With the elimination: the columns are the
  // reduced matrix's, and a requested e-block selects all of F(e) in its place
  std::vector<int> sel_of(num_pb, -1);
  C.sel_off.push_back(0);
  auto select_cb = [&](int cb) {
    const int b = T.cb_block[cb];
    if (sel_of[b] >= 0) return;
    sel_of[b] = (int)C.sel_cb.size();
    C.sel_cb.push_back(cb);
    for (int j = 0; j < T.cb_size[cb]; ++j) C.sel_col.push_back((schur ? C.cb_red[cb] : T.cb_col[cb]) + j);
    C.sel_off.push_back((int)C.sel_col.size());
  };
  auto select = [&](int b) {
    if (T.cb_of[b] < 0) return;
    if (!schur || !C.cb_elim[T.cb_of[b]]) { select_cb(T.cb_of[b]); return; }
    const int e = C.cb_red[T.cb_of[b]];
    for (int k = C.ew_begin[e]; k < C.ew_begin[e + 1]; ++k) { select_cb(C.ew_g[k]); C.ew_sel[k] = C.sel_off[sel_of[T.cb_block[C.ew_g[k]]]]; }
  };
  std::map<std::pair<int, int>, int> seen;
  for (const auto& ab : pairs) {
    if (ab.first < 0 || ab.first >= num_pb || ab.second < 0 || ab.second >= num_pb) {
      if (why) *why = "Covariance: a requested block is no parameter block of the problem";
      return SK_ERR_INVALID_ARGUMENT;
    }
    select(ab.first); select(ab.second);
    const std::pair<int, int> key(std::min(ab.first, ab.second), std::max(ab.first, ab.second));
    if (!seen.emplace(key, (int)C.req_a.size()).second) continue;
    C.req_a.push_back(key.first); C.req_b.push_back(key.second);
  }
  C.k = (int)C.sel_col.size();
  for (size_t r = 0; r < C.req_a.size(); ++r) {
    const int a = C.req_a[r], b = C.req_b[r];
    const bool zero = T.cb_of[a] < 0 || T.cb_of[b] < 0;
    const bool ea = schur && !zero && C.cb_elim[T.cb_of[a]], eb = schur && !zero && C.cb_elim[T.cb_of[b]];
    C.req_ra.push_back(zero ? -1 : ea ? 0 : C.sel_off[sel_of[a]]);
    C.req_rb.push_back(zero ? -1 : eb ? 0 : C.sel_off[sel_of[b]]);
    if (schur) { C.req_ea.push_back(ea ? C.cb_red[T.cb_of[a]] : -1); C.req_eb.push_back(eb ? C.cb_red[T.cb_of[b]] : -1); }
    C.req_tan_off.push_back(C.out_size); C.out_size += (long)T.pb_local_size[a] * T.pb_local_size[b];
    C.req_amb_off.push_back(C.out_size); C.out_size += (long)T.pb_size[a] * T.pb_size[b];
  }
  return SK_OK;
}

}  // namespace sk
