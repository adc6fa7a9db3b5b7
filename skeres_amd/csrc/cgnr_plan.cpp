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

int cgnr_plan_build(const Problem& p, CgnrPlan* plan, std::string* why) {
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
  return SK_OK;
}

}  // namespace sk
