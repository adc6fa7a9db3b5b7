// Tangent columns, parts and the block-size refusal — see jacobian_plan.hpp.  No HIP in this file.
#include "jacobian_plan.hpp"

#include <algorithm>
#include <cstdio>

namespace sk {

void tangent_columns_build(const Problem& p, const EvaluatePlan& E, ConstantTangent constants, TangentColumns* columns) {
  TangentColumns& T = *columns;
  T = TangentColumns();
  const int num_pb = (int)p.block_ptr.size();
  T.block_off.assign(num_pb + 1, 0);
  T.pb_type.resize(num_pb); T.pb_size.resize(num_pb); T.pb_local_size.resize(num_pb); T.pb_local_off.assign(num_pb, -1); T.pb_mask.resize(num_pb);
  T.cb_of.assign(num_pb, -1);
  int cols = 0;
  for (int b = 0; b < num_pb; ++b) {
    T.block_off[b + 1] = T.block_off[b] + p.block_size[b];
    const int pz = b < (int)p.block_param.size() ? p.block_param[b] : -1;
    const bool constant = b < (int)p.block_constant.size() && p.block_constant[b];
    T.pb_type[b] = constant ? (int)kParamConstant : pz >= 0 ? p.params[pz].type : (int)kParamIdentity;
    T.pb_mask[b] = pz >= 0 ? p.params[pz].constant_mask : 0u;
    T.pb_size[b] = p.block_size[b];
    T.pb_local_size[b] = constant && constants == ConstantTangent::kZero ? 0 : E.col_size[b];
    if (constant || E.col_size[b] == 0) continue;
    T.pb_local_off[b] = cols;
    T.cb_of[b] = (int)T.cb_col.size();
    T.cb_col.push_back(cols); T.cb_size.push_back(E.col_size[b]); T.cb_block.push_back(b);
    cols += E.col_size[b];
  }
  T.num_cols = cols;
  T.num_ambient = T.block_off[num_pb];
}

void cut_parts(const std::vector<int>& begin_of, PartList* parts) {
  PartList& L = *parts;
  L = PartList();
  const int owners = (int)begin_of.size() - 1;
  L.long_begin.push_back(0);
  for (int q = 0; q < owners; ++q) {
    const int begin = begin_of[q], end = begin_of[q + 1];
    const int nparts = std::max(1, (end - begin + kCgnrPartSlots - 1) / kCgnrPartSlots);
    for (int k = 0; k < nparts; ++k) {
      L.owner.push_back(q);
      L.begin.push_back(begin + k * kCgnrPartSlots);
      L.end.push_back(std::min(end, begin + (k + 1) * kCgnrPartSlots));
      L.out.push_back(nparts == 1 ? -1 : L.num_partials++);
    }
    if (nparts > 1) { L.long_owner.push_back(q); L.long_begin.push_back(L.num_partials); }
  }
}

void greedy_independent_set(const std::vector<int>& nb_begin, const std::vector<int>& nb, std::vector<int>* in_set) {
  const int ncb = (int)nb_begin.size() - 1;
  std::vector<int> order(ncb);
  for (int c = 0; c < ncb; ++c) order[c] = c;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return nb_begin[a + 1] - nb_begin[a] < nb_begin[b + 1] - nb_begin[b]; });
  in_set->assign(ncb, 0);
  for (int c : order) {
    bool free = true;
    for (int k = nb_begin[c]; k < nb_begin[c + 1] && free; ++k) free = !(*in_set)[nb[k]];
    (*in_set)[c] = free ? 1 : 0;
  }
}

std::string block_size_refusal(const Problem& p, const char* feature, int limit, bool constants_too) {
  char buf[256];
  for (size_t b = 0; b < p.block_size.size(); ++b) {
    if (!constants_too && b < p.block_constant.size() && p.block_constant[b]) continue;
    const int pz = b < p.block_param.size() ? p.block_param[b] : -1;
    const int tangent = pz >= 0 ? p.params[pz].local_size : p.block_size[b];
    if (pz >= 0 && p.block_size[b] > limit) {
      snprintf(buf, sizeof(buf), "%s takes parameterized blocks of size up to %d (parameter block %d has %d: not supported)", feature, limit, (int)b, p.block_size[b]);
      return buf;
    }
    if (tangent > limit) {
      snprintf(buf, sizeof(buf), "%s takes parameter blocks of tangent size up to %d (parameter block %d has %d: not supported)", feature, limit, (int)b, tangent);
      return buf;
    }
  }
  return "";
}

}  // namespace sk
