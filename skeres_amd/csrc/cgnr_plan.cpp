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
  for (size_t b = 0; b < p.block_size.size(); ++b) {
    if (b < p.block_constant.size() && p.block_constant[b]) continue;
    const int pz = b < p.block_param.size() ? p.block_param[b] : -1;
    const int tangent = pz >= 0 ? p.params[pz].local_size : p.block_size[b];
    if (pz >= 0 && p.block_size[b] > kCgnrMaxBlock) {
      snprintf(buf, sizeof(buf), "CGNR takes parameterized blocks of size up to %d (parameter block %d has %d: not supported)", kCgnrMaxBlock, (int)b, p.block_size[b]);
      return buf;
    }
    if (tangent > kCgnrMaxBlock) {
      snprintf(buf, sizeof(buf), "CGNR takes parameter blocks of tangent size up to %d (parameter block %d has %d: not supported)", kCgnrMaxBlock, (int)b, tangent);
      return buf;
    }
  }
  return "";
}

int cgnr_plan_build(const Problem& p, CgnrPlan* plan, std::string* why) {
  CgnrPlan& C = *plan;
  C = CgnrPlan();
  int rc = evaluate_plan_build(p, nullptr, false, false, true, &C.eval, why);
  if (rc != SK_OK) return rc;
  {  // the staging of a residual-only evaluation: the same groups, num_residuals planes each
    EvaluatePlan cost;
    rc = evaluate_plan_build(p, nullptr, false, false, false, &cost, why);
    if (rc != SK_OK) return rc;
    C.blk_stage_cost = cost.blk_stage;
    for (const EvaluateGroup& G : cost.groups) C.group_stage_cost.push_back(G.stage_off);
  }
  const EvaluatePlan& E = C.eval;
  const int num_pb = (int)p.block_ptr.size(), nb = (int)E.blocks.size(), ns = (int)E.slot_block.size();

  C.block_off.assign(num_pb + 1, 0);
  C.pb_type.resize(num_pb); C.pb_local_size.resize(num_pb); C.pb_local_off.resize(num_pb); C.pb_mask.resize(num_pb);
  std::vector<int> cb_of(num_pb, -1);
  C.cb_moff.push_back(0);
  long long cols = 0;
  for (int b = 0; b < num_pb; ++b) {
    C.block_off[b + 1] = C.block_off[b] + p.block_size[b];
    const int pz = b < (int)p.block_param.size() ? p.block_param[b] : -1;
    const bool constant = b < (int)p.block_constant.size() && p.block_constant[b];
    C.pb_type[b] = constant ? (int)kParamConstant : pz >= 0 ? p.params[pz].type : (int)kParamIdentity;
    C.pb_mask[b] = pz >= 0 ? p.params[pz].constant_mask : 0u;
    C.pb_local_size[b] = constant ? 0 : E.col_size[b];
    C.pb_local_off[b] = C.pb_local_size[b] > 0 ? (int)cols : -1;
    if (C.pb_local_size[b] == 0) continue;
    cb_of[b] = (int)C.cb_col.size();
    C.cb_col.push_back((int)cols); C.cb_size.push_back(C.pb_local_size[b]); C.cb_block.push_back(b);
    C.cb_moff.push_back(C.cb_moff.back() + C.pb_local_size[b] * C.pb_local_size[b]);
    cols += C.pb_local_size[b];
  }
  C.num_cols = (int)cols;
  C.num_ambient = C.block_off[num_pb];

  C.slot_col.assign(ns, -1); C.slot_size.assign(ns, 0);
  const int ncb = (int)C.cb_col.size();
  C.cb_begin.assign(ncb + 1, 0);
  for (int s = 0; s < ns; ++s) {
    if (E.slot_pos[s] < 0) continue;
    const int b = E.slot_block[s];
    C.slot_col[s] = C.pb_local_off[b]; C.slot_size[s] = C.pb_local_size[b];
    ++C.cb_begin[cb_of[b] + 1];
  }
  for (int c = 0; c < ncb; ++c) C.cb_begin[c + 1] += C.cb_begin[c];
  C.cb_slots.resize(C.cb_begin[ncb]);
  {
    std::vector<int> fill(C.cb_begin.begin(), C.cb_begin.end() - 1);
    for (int s = 0; s < ns; ++s) if (E.slot_pos[s] >= 0) C.cb_slots[fill[cb_of[E.slot_block[s]]]++] = s;  // slots ascend with the rows
  }

  C.row_block.resize((size_t)E.num_rows);
  for (int i = 0; i < nb; ++i) for (int r = E.row_off[i]; r < E.row_off[i + 1]; ++r) C.row_block[r] = i;

  // parts: kCgnrPartSlots slots each, the last of a block shorter; a block without slots (nothing observes it) has one empty part
  C.long_begin.push_back(0);
  for (int c = 0; c < ncb; ++c) {
    const int begin = C.cb_begin[c], end = C.cb_begin[c + 1];
    const int nparts = std::max(1, (end - begin + kCgnrPartSlots - 1) / kCgnrPartSlots);
    for (int k = 0; k < nparts; ++k) {
      C.part_cb.push_back(c);
      C.part_begin.push_back(begin + k * kCgnrPartSlots);
      C.part_end.push_back(std::min(end, begin + (k + 1) * kCgnrPartSlots));
      C.part_out.push_back(nparts == 1 ? -1 : C.num_partials++);
    }
    if (nparts > 1) { C.long_cb.push_back(c); C.long_begin.push_back(C.num_partials); }
  }
  return SK_OK;
}

}  // namespace sk
