// Host plan of Problem::Evaluate — see evaluate_plan.hpp.  No HIP in this file.
#include "evaluate_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <map>
#include <utility>

namespace sk {

namespace {
int fail(std::string* why, int status, const char* fmt, long long a = 0, long long b = 0) {
  char buf[256];
  snprintf(buf, sizeof(buf), fmt, a, b);
  if (why) *why = buf;
  return status;
}
}  // namespace

size_t evaluate_plan_staging(const EvaluatePlan& plan, bool jacobian, std::vector<size_t>* group_stage, std::vector<size_t>* blk_stage, std::vector<int>* blk_stride) {
  size_t stage = 0;
  group_stage->clear();
  blk_stage->resize(plan.blocks.size());
  if (blk_stride) blk_stride->resize(plan.blocks.size());
  for (const EvaluateGroup& G : plan.groups) {
    group_stage->push_back(stage);
    const size_t count = G.members.size();
    for (size_t l = 0; l < count; ++l) { (*blk_stage)[G.members[l]] = stage + l; if (blk_stride) (*blk_stride)[G.members[l]] = (int)count; }
    stage += count * (size_t)G.num_residuals * (size_t)(jacobian ? 1 + G.dim : 1);
  }
  return stage;
}

int evaluate_plan_build(const Problem& p, const EvaluateOptions* options, bool structure, bool gradient, bool jacobian, EvaluatePlan* plan,
                        std::string* why) {
  static const EvaluateOptions kDefaults;
  const EvaluateOptions& o = options ? *options : kDefaults;
  EvaluatePlan& P = *plan;
  P = EvaluatePlan();
  const int num_rb = (int)p.rb_functor.size(), num_pb = (int)p.block_ptr.size();
  for (int b = 0; b < num_rb; ++b)
    if (p.rb_functor[b] == SK_FUNCTOR_SYNTH_TANH_ROW)
      return fail(why, SK_ERR_UNSUPPORTED, "Evaluate: a problem with dense rows (sk_problem_add_dense_rows) has a dense Jacobian; not offered");

  // columns
  P.col_off.assign(num_pb, -1);
  P.col_size.resize(num_pb);
  for (int b = 0; b < num_pb; ++b) {
    const int pz = b < (int)p.block_param.size() ? p.block_param[b] : -1;
    P.col_size[b] = pz >= 0 ? p.params[pz].local_size : p.block_size[b];
  }
  std::vector<int> column_blocks;
  if (o.parameter_blocks.empty()) {
    for (int b = 0; b < num_pb; ++b) column_blocks.push_back(b);
  } else {
    std::vector<char> seen(num_pb, 0);
    for (size_t i = 0; i < o.parameter_blocks.size(); ++i) {
      auto it = p.block_of.find(o.parameter_blocks[i]);
      if (it == p.block_of.end()) return fail(why, SK_ERR_INVALID_ARGUMENT, "Evaluate: parameter_blocks[%lld] is no parameter block of the problem", (long long)i);
      if (seen[it->second]) return fail(why, SK_ERR_INVALID_ARGUMENT, "Evaluate: parameter_blocks[%lld] is listed twice", (long long)i);
      seen[it->second] = 1;
      column_blocks.push_back(it->second);
    }
  }
  long long cols = 0;
  for (int b : column_blocks) {
    P.col_off[b] = (int)cols;
    cols += P.col_size[b];
    if (cols >= (1ll << 31)) return fail(why, SK_ERR_UNSUPPORTED, "Evaluate: 2^31 columns or more");
  }
  P.num_cols = (int)cols;

  // rows
  if (o.residual_blocks.empty()) {
    P.blocks.resize(num_rb);
    for (int b = 0; b < num_rb; ++b) P.blocks[b] = b;
  } else {
    std::vector<char> seen(num_rb, 0);
    for (size_t i = 0; i < o.residual_blocks.size(); ++i) {
      const int id = o.residual_blocks[i];
      if (id < 0 || id >= num_rb) return fail(why, SK_ERR_INVALID_ARGUMENT, "Evaluate: residual_blocks[%lld] = %lld is no residual block of the problem", (long long)i, id);
      if (seen[id]) return fail(why, SK_ERR_INVALID_ARGUMENT, "Evaluate: residual block %lld is listed twice", id);
      seen[id] = 1;
    }
    P.blocks = o.residual_blocks;
  }
  const int nb = (int)P.blocks.size();
  P.row_off.resize(nb + 1); P.val_off.resize(nb + 1); P.slot_begin.resize(nb + 1);
  long long rows = 0, nnz = 0;
  std::map<int, int> group_of;       // functor -> group
  std::vector<int> callback_blocks;  // listed positions
  std::vector<std::pair<int, int>> order;  // (column, slot) of the stored slots of one block
  for (int i = 0; i < nb; ++i) {
    const int b = P.blocks[i], nres = p.rb_num_residuals[b];
    P.row_off[i] = (int)rows; P.val_off[i] = (int)nnz; P.slot_begin[i] = (int)P.slot_block.size();
    int k0 = 0;
    order.clear();
    for (size_t q = p.rb_pidx_off[b]; q < p.rb_pidx_off[b + 1]; ++q) {
      const int pb = p.rb_pidx[q];
      const bool constant = pb < (int)p.block_constant.size() && p.block_constant[pb];
      const int s = (int)P.slot_block.size();
      P.slot_block.push_back(pb); P.slot_k0.push_back(k0); P.slot_owner.push_back(i);
      P.slot_pos.push_back(-1);
      if (P.col_off[pb] >= 0 && !constant && P.col_size[pb] > 0) order.emplace_back(P.col_off[pb], s);
      k0 += p.block_size[pb];
    }
    std::sort(order.begin(), order.end());  // within a row the columns ascend
    int width = 0;
    for (const auto& cs : order) { P.slot_pos[cs.second] = width; width += P.col_size[P.slot_block[cs.second]]; }
    rows += nres; nnz += (long long)nres * width;
    if (rows >= (1ll << 31) || nnz >= (1ll << 31)) return fail(why, SK_ERR_UNSUPPORTED, "Evaluate: a Jacobian with 2^31 rows or stored entries or more does not fit ceres::CRSMatrix's 32-bit indices");
    const int f = p.rb_functor[b];
    if (f == SK_FUNCTOR_HOST_CALLBACK) { callback_blocks.push_back(i); continue; }
    group_of.emplace(f, 0);  // numbered below, in functor order
  }
  P.row_off[nb] = (int)rows; P.val_off[nb] = (int)nnz; P.slot_begin[nb] = (int)P.slot_block.size();
  P.num_rows = (int)rows; P.num_nonzeros = nnz;

  // evaluation groups and their staging
  int g = 0;
  for (auto& kv : group_of) { kv.second = g++; P.groups.emplace_back(); P.groups.back().functor = kv.first; }
  auto dim_of = [&](int i) { int d = 0; for (int s = P.slot_begin[i]; s < P.slot_begin[i + 1]; ++s) d += p.block_size[P.slot_block[s]]; return d; };
  for (int i = 0; i < nb; ++i) {
    const int f = p.rb_functor[P.blocks[i]];
    if (f == SK_FUNCTOR_HOST_CALLBACK) continue;
    EvaluateGroup& G = P.groups[group_of[f]];
    if (G.members.empty()) { G.num_residuals = p.rb_num_residuals[P.blocks[i]]; G.dim = dim_of(i); }
    G.members.push_back(i);
  }
  for (int i : callback_blocks) {
    P.groups.emplace_back();
    EvaluateGroup& G = P.groups.back();
    G.functor = SK_FUNCTOR_HOST_CALLBACK; G.num_residuals = p.rb_num_residuals[P.blocks[i]]; G.dim = dim_of(i); G.members.push_back(i);
  }
  std::vector<size_t> group_stage;
  P.stage_size = evaluate_plan_staging(P, jacobian, &group_stage, &P.blk_stage, &P.blk_stride);
  bool in_callbacks = false;
  for (size_t g = 0; g < P.groups.size(); ++g) {
    EvaluateGroup& G = P.groups[g];
    G.stage_off = group_stage[g];
    if (G.functor == SK_FUNCTOR_HOST_CALLBACK && !in_callbacks) { in_callbacks = true; P.callback_stage_begin = G.stage_off; }
  }
  if (!in_callbacks) P.callback_stage_begin = P.stage_size;

  if (gradient) {
    std::vector<int> cb_of(num_pb, -1);
    for (int b : column_blocks) {
      cb_of[b] = (int)P.grad_col.size();
      P.grad_col.push_back(P.col_off[b]); P.grad_size.push_back(P.col_size[b]);
    }
    const int ncb = (int)P.grad_col.size();
    P.grad_begin.assign(ncb + 1, 0);
    const int ns = (int)P.slot_block.size();
    for (int s = 0; s < ns; ++s) if (P.slot_pos[s] >= 0) ++P.grad_begin[cb_of[P.slot_block[s]] + 1];
    for (int c = 0; c < ncb; ++c) P.grad_begin[c + 1] += P.grad_begin[c];
    P.grad_slots.resize(P.grad_begin[ncb]);
    std::vector<int> fill(P.grad_begin.begin(), P.grad_begin.end() - 1);
    for (int s = 0; s < ns; ++s) if (P.slot_pos[s] >= 0) P.grad_slots[fill[cb_of[P.slot_block[s]]]++] = s;  // slots ascend with the rows
  }

  if (structure) {
    P.rows.resize((size_t)P.num_rows + 1);
    P.cols.resize((size_t)nnz);
    for (int i = 0; i < nb; ++i) {
      const int nres = P.row_off[i + 1] - P.row_off[i];
      const int width = nres > 0 ? (P.val_off[i + 1] - P.val_off[i]) / nres : 0;
      for (int r = 0; r < nres; ++r) {
        const int first = P.val_off[i] + r * width;
        P.rows[P.row_off[i] + r] = first;
        for (int s = P.slot_begin[i]; s < P.slot_begin[i + 1]; ++s) {
          if (P.slot_pos[s] < 0) continue;
          const int c0 = P.col_off[P.slot_block[s]], w = P.col_size[P.slot_block[s]];
          for (int j = 0; j < w; ++j) P.cols[(size_t)first + P.slot_pos[s] + j] = c0 + j;
        }
      }
    }
    P.rows[P.num_rows] = (int)nnz;
  }
  return SK_OK;
}

}  // namespace sk
