// Inner iterations on the device — see inner_iterations.hpp.
#include "inner_iterations.hpp"

#include <algorithm>

#include "dev_knobs.hpp"

namespace sk {

InnerIterations::~InnerIterations() {
  for (Group* g : groups_) delete g;
  if (h_flags_) (void)hipHostFree(h_flags_);
}

int InnerIterations::setup(const InnerPlan& plan, const Shared& shared, hipStream_t s) {
  sh_ = shared; s_ = s;
  refined_pb_.assign((size_t)sh_.num_pb, 0);
  for (const InnerGroup& G : plan.groups) {
    Group* g = new Group();
    groups_.push_back(g);
    const CgnrColumnSubset& S = G.blocks;
    const PartList& L = S.parts;
    SK_HIP_TRY(upload_padded(g->b[0], S.cb_col, s)); SK_HIP_TRY(upload_padded(g->b[1], S.cb_size, s)); SK_HIP_TRY(upload_padded(g->b[2], S.cb_moff, s));
    SK_HIP_TRY(upload_padded(g->b[3], S.cb_slots, s));
    SK_HIP_TRY(upload_padded(g->b[4], L.owner, s)); SK_HIP_TRY(upload_padded(g->b[5], L.begin, s)); SK_HIP_TRY(upload_padded(g->b[6], L.end, s)); SK_HIP_TRY(upload_padded(g->b[7], L.out, s));
    SK_HIP_TRY(upload_padded(g->b[8], L.long_owner, s)); SK_HIP_TRY(g->b[9].upload(L.long_begin, s));
    SK_HIP_TRY(upload_padded(g->pb, G.pb, s)); SK_HIP_TRY(upload_padded(g->cost_rb, G.cost_rb, s));
    CgnrCols& C = g->dev.cols;
    C.num_cb = (int)S.cb.size(); C.num_parts = (int)L.owner.size(); C.num_long = (int)L.long_owner.size();
    C.cb_col = g->b[0].p; C.cb_size = g->b[1].p; C.cb_moff = g->b[2].p; C.cb_slots = g->b[3].p;
    C.part_cb = g->b[4].p; C.part_begin = g->b[5].p; C.part_end = g->b[6].p; C.part_out = g->b[7].p;
    C.long_cb = g->b[8].p; C.long_begin = g->b[9].p;
    g->dev.pb = g->pb.p; g->dev.cost_rb = g->cost_rb.p;
    for (int pb : G.pb) refined_pb_[pb] = 1;
  }
  SK_HIP_TRY(b_xc_.alloc((size_t)sh_.num_ambient));
  SK_HIP_TRY(b_st_.alloc((size_t)sh_.num_pb * kInDCount)); SK_HIP_TRY(b_st_.zero(s));
  SK_HIP_TRY(b_sti_.alloc((size_t)sh_.num_pb * kInICount)); SK_HIP_TRY(b_sti_.zero(s));
  SK_HIP_TRY(b_scale_.alloc((size_t)sh_.num_cols)); SK_HIP_TRY(b_g_.alloc((size_t)sh_.num_cols)); SK_HIP_TRY(b_H_.alloc(sh_.matrix_entries));
  const size_t blocks = (size_t)std::max(plan.max_group_blocks, 1);
  SK_HIP_TRY(b_csum_.alloc(blocks)); SK_HIP_TRY(b_csum_c_.alloc(blocks));
  SK_HIP_TRY(b_cost_partial_.alloc((size_t)std::max(plan.max_partials, 1)));
  SK_HIP_TRY(b_flags_.alloc(kInFlagCount)); SK_HIP_TRY(b_flags_.zero(s));
  SK_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_flags_), kInFlagCount * sizeof(int), hipHostMallocDefault));
  dev_.st = b_st_.p; dev_.sti = b_sti_.p; dev_.scale = b_scale_.p; dev_.g = b_g_.p; dev_.H = b_H_.p;
  dev_.csum = b_csum_.p; dev_.csum_c = b_csum_c_.p; dev_.cost_partial = b_cost_partial_.p; dev_.flags = b_flags_.p;
  return SK_OK;
}

// One round of a group (inner_iterations.hpp): x_dev is the point, b_xc_ the second point.
int InnerIterations::round(const Group& G, double* x_dev) {
  hipStream_t s = s_;
  DeviceJacobian& dj = *sh_.dj;
  const int* flags = b_flags_.p;
  int rc = dj.evaluate(x_dev, true);
  if (rc) return rc;
  dj.finish(x_dev, sh_.r, sh_.jac.values, sh_.cterm);
  launch_cgnr_jtw(kCgnrJtwPlain, sh_.jac, G.dev.cols, sh_.r, nullptr, nullptr, nullptr, nullptr, b_g_.p, sh_.jtw_partial, flags, s);
  launch_cgnr_block_diag(sh_.jac, G.dev.cols, b_H_.p, sh_.bd_partial, s, flags);
  launch_inner_cost(G.dev, dev_, sh_.cterm, b_csum_.p, s);
  launch_inner_step(G.dev, dev_, dj.pblocks(), x_dev, b_xc_.p, s);
  rc = dj.evaluate(b_xc_.p, false, sh_.group_stage_cost);
  if (rc) return rc;
  dj.finish(b_xc_.p, sh_.rc, nullptr, sh_.cterm_c, sh_.blk_stage_cost);
  launch_inner_cost(G.dev, dev_, sh_.cterm_c, b_csum_c_.p, s);
  launch_inner_accept(G.dev, dev_, dj.pblocks(), x_dev, b_xc_.p, s);
  launch_inner_round_end(dev_, s);
  return SK_OK;
}

int InnerIterations::refine(double* x_dev, int* rounds) {
  hipStream_t s = s_;
  *rounds = 0;
  const int batch = dev_knobs().inner_batch > 0 ? dev_knobs().inner_batch : inner::kBatch;
  // a running block spends an iteration in every round, so a group is done after kMaxNumIterations + 1 rounds at the latest
  const int max_rounds = inner::kMaxNumIterations + 2;
  for (const Group* G : groups_) {
    if (G->dev.cols.num_cb == 0) continue;
    launch_inner_begin(G->dev, dev_, s);
    SK_HIP_TRY(hipMemcpyAsync(b_xc_.p, x_dev, (size_t)sh_.num_ambient * sizeof(double), hipMemcpyDeviceToDevice, s));
    int enqueued = 0;
    for (;;) {
      for (int k = 0; k < batch && enqueued < max_rounds; ++k, ++enqueued) { const int rc = round(*G, x_dev); if (rc) return rc; }
      SK_HIP_TRY(hipMemcpyAsync(h_flags_, b_flags_.p, kInFlagCount * sizeof(int), hipMemcpyDeviceToHost, s));
      SK_HIP_TRY(hipStreamSynchronize(s));
      if (h_flags_[kInDone] || enqueued >= max_rounds) break;
    }
    SK_HIP_TRY(hipGetLastError());
    *rounds += h_flags_[kInRounds];
  }
  refined_once_ = true;
  return SK_OK;
}

int InnerIterations::blocks(int* iterations, int* status) {
  std::vector<int> h((size_t)sh_.num_pb * kInICount);
  SK_HIP_TRY(hipMemcpyAsync(h.data(), b_sti_.p, h.size() * sizeof(int), hipMemcpyDeviceToHost, s_));
  SK_HIP_TRY(hipStreamSynchronize(s_));
  for (int b = 0; b < sh_.num_pb; ++b) {
    const bool have = refined_once_ && refined_pb_[b];
    if (iterations) iterations[b] = have ? h[(size_t)b * kInICount + kInIters] : -1;
    if (status) status[b] = have ? h[(size_t)b * kInICount + kInStatus] : -1;
  }
  return SK_OK;
}

}  // namespace sk
