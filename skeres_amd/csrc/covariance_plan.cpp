// Host plan of sk_covariance_compute — see covariance_plan.hpp.  No HIP in this file.
#include "covariance_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <map>

namespace sk {

namespace {
int tangent_of(const Problem& p, size_t b) {
  const int pz = b < p.block_param.size() ? p.block_param[b] : -1;
  return pz >= 0 ? p.params[pz].local_size : p.block_size[b];
}
}  // namespace

std::string covariance_refusal(const Problem& p) {
  char buf[320];
  for (size_t b = 0; b < p.rb_functor.size(); ++b)
    if (p.rb_functor[b] == SK_FUNCTOR_SYNTH_TANH_ROW)
      return "Covariance works on a block-sparse Jacobian: dense-row problems (sk_problem_add_dense_rows) are not supported";
  long long cols = 0;
  for (size_t b = 0; b < p.block_size.size(); ++b) {
    const int pz = b < p.block_param.size() ? p.block_param[b] : -1;
    const int tangent = tangent_of(p, b);
    if (pz >= 0 && p.block_size[b] > kCovarianceMaxBlock) {
      snprintf(buf, sizeof(buf), "Covariance takes parameterized blocks of size up to %d (parameter block %d has %d: not supported)", kCovarianceMaxBlock, (int)b, p.block_size[b]);
      return buf;
    }
    if (tangent > kCovarianceMaxBlock) {
      snprintf(buf, sizeof(buf), "Covariance takes parameter blocks of tangent size up to %d (parameter block %d has %d: not supported)", kCovarianceMaxBlock, (int)b, tangent);
      return buf;
    }
    if (!(b < p.block_constant.size() && p.block_constant[b])) cols += tangent;
  }
  if (cols > kCovarianceMaxColumns) {
    snprintf(buf, sizeof(buf),
             "Covariance factors the dense normal matrix of the whole problem and takes up to %d columns (this problem has %lld: not supported); the "
             "bundle-adjustment route through the reduced camera system is not built",
             kCovarianceMaxColumns, cols);
    return buf;
  }
  return "";
}

int covariance_plan_build(const Problem& p, const std::vector<std::pair<int, int>>& pairs, CovariancePlan* plan, std::string* why) {
  CovariancePlan& C = *plan;
  C = CovariancePlan();
  const std::string refusal = covariance_refusal(p);
  if (!refusal.empty()) { if (why) *why = refusal; return SK_ERR_UNSUPPORTED; }
  int rc = evaluate_plan_build(p, nullptr, false, false, true, &C.eval, why);
  if (rc != SK_OK) return rc;
  const EvaluatePlan& E = C.eval;
  const int num_pb = (int)p.block_ptr.size(), nb = (int)E.blocks.size();

  // columns: the parameter blocks that move, as cgnr_plan_build takes them
  C.block_off.assign(num_pb + 1, 0);
  C.pb_type.resize(num_pb); C.pb_size.resize(num_pb); C.pb_local_size.resize(num_pb); C.pb_local_off.assign(num_pb, -1); C.pb_mask.resize(num_pb);
  std::vector<int> cb_of(num_pb, -1);
  int cols = 0;
  for (int b = 0; b < num_pb; ++b) {
    C.block_off[b + 1] = C.block_off[b] + p.block_size[b];
    const int pz = b < (int)p.block_param.size() ? p.block_param[b] : -1;
    const bool constant = b < (int)p.block_constant.size() && p.block_constant[b];
    C.pb_type[b] = constant ? (int)kParamConstant : pz >= 0 ? p.params[pz].type : (int)kParamIdentity;
    C.pb_mask[b] = pz >= 0 ? p.params[pz].constant_mask : 0u;
    C.pb_size[b] = p.block_size[b];
    C.pb_local_size[b] = E.col_size[b];
    if (constant || E.col_size[b] == 0) continue;
    C.pb_local_off[b] = cols;
    cb_of[b] = (int)C.cb_col.size();
    C.cb_col.push_back(cols); C.cb_size.push_back(E.col_size[b]); C.cb_block.push_back(b);
    cols += E.col_size[b];
  }
  C.num_cols = cols;
  const int ncb = (int)C.cb_col.size();

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
        const int ci = cb_of[E.slot_block[s]], cj = cb_of[E.slot_block[t]];
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

  // parts: kCgnrPartSlots terms each, exactly as cgnr_plan_build cuts the slot lists
  const int npairs = (int)C.pair_i.size();
  C.long_begin.push_back(0);
  for (int q = 0; q < npairs; ++q) {
    const int begin = C.pair_begin[q], end = C.pair_begin[q + 1];
    const int nparts = std::max(1, (end - begin + kCgnrPartSlots - 1) / kCgnrPartSlots);
    for (int k = 0; k < nparts; ++k) {
      C.part_pair.push_back(q);
      C.part_begin.push_back(begin + k * kCgnrPartSlots);
      C.part_end.push_back(std::min(end, begin + (k + 1) * kCgnrPartSlots));
      C.part_out.push_back(nparts == 1 ? -1 : C.num_partials++);
    }
    if (nparts > 1) { C.long_pair.push_back(q); C.long_begin.push_back(C.num_partials); }
  }

  // the selection, in order of first appearance, and the requested pairs, each once
  std::vector<int> sel_of(num_pb, -1);
  C.sel_off.push_back(0);
  auto select = [&](int b) {
    if (cb_of[b] < 0 || sel_of[b] >= 0) return;
    sel_of[b] = (int)C.sel_cb.size();
    C.sel_cb.push_back(cb_of[b]);
    for (int j = 0; j < C.cb_size[cb_of[b]]; ++j) C.sel_col.push_back(C.cb_col[cb_of[b]] + j);
    C.sel_off.push_back((int)C.sel_col.size());
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
    const bool zero = sel_of[a] < 0 || sel_of[b] < 0;
    C.req_ra.push_back(zero ? -1 : C.sel_off[sel_of[a]]);
    C.req_rb.push_back(zero ? -1 : C.sel_off[sel_of[b]]);
    C.req_tan_off.push_back(C.out_size); C.out_size += (long)C.pb_local_size[a] * C.pb_local_size[b];
    C.req_amb_off.push_back(C.out_size); C.out_size += (long)C.pb_size[a] * C.pb_size[b];
  }
  return SK_OK;
}

}  // namespace sk
