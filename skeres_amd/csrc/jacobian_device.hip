// The device image of a Problem and its EvaluatePlan — see jacobian_device.hpp.
#include "jacobian_device.hpp"

#include <algorithm>
#include <cstring>

namespace sk {

std::vector<ParamBlock> param_blocks(const Problem& p, const EvaluatePlan& P, const TangentColumns* T) {
  const int num_pb = (int)p.block_ptr.size();
  std::vector<ParamBlock> pblocks((size_t)std::max(num_pb, 1));
  int off = 0;
  for (int b = 0; b < num_pb; ++b) {
    ParamBlock& pb = pblocks[b];
    const int pz = b < (int)p.block_param.size() ? p.block_param[b] : -1;
    pb.type = T ? T->pb_type[b] : pz >= 0 ? p.params[pz].type : kParamIdentity;
    pb.global_size = p.block_size[b]; pb.local_size = T ? T->pb_local_size[b] : P.col_size[b];
    pb.constant_mask = pz >= 0 ? p.params[pz].constant_mask : 0u;
    pb.global_off = off; pb.local_off = T ? T->pb_local_off[b] : P.col_off[b];
    off += p.block_size[b];
  }
  return pblocks;
}

void DeviceJacobian::gather(const Problem& p, const EvaluatePlan& P, std::vector<ParamBlock> pblocks, bool apply_loss) {
  p_ = &p; P_ = &P;
  const int nb = (int)P.blocks.size(), num_pb = (int)p.block_ptr.size();
  // the point: the caller's parameter memory, now
  h_block_off_.assign(num_pb + 1, 0);
  for (int b = 0; b < num_pb; ++b) h_block_off_[b + 1] = h_block_off_[b] + p.block_size[b];
  h_x_.assign((size_t)std::max(h_block_off_[num_pb], 1), 0.0);
  for (int b = 0; b < num_pb; ++b) std::memcpy(&h_x_[h_block_off_[b]], p.block_ptr[b], p.block_size[b] * sizeof(double));
  h_xoff_.resize(p.rb_pidx.size());
  for (size_t i = 0; i < p.rb_pidx.size(); ++i) h_xoff_[i] = h_block_off_[p.rb_pidx[i]];
  h_pblocks_ = std::move(pblocks);
  h_blk_dim_.assign(std::max(nb, 1), 0); h_blk_loss_.assign(std::max(nb, 1), -1);
  h_members_.clear(); member_off_.clear();
  for (const EvaluateGroup& G : P.groups) {
    member_off_.push_back(h_members_.size());
    h_members_.insert(h_members_.end(), G.members.begin(), G.members.end());
    for (int i : G.members) h_blk_dim_[i] = G.dim;
  }
  if (apply_loss) for (int i = 0; i < nb; ++i) h_blk_loss_[i] = p.rb_loss[P.blocks[i]];
  h_cb_stage_.assign(P.stage_size - P.callback_stage_begin, 0.0);
  h_nodes_ = loss_nodes_or_trivial(p.loss_nodes);
}

int DeviceJacobian::upload(bool want_values, bool by_column, hipStream_t s) {
  const Problem& p = *p_;
  const EvaluatePlan& P = *P_;
  s_ = s;
  SK_HIP_TRY(x_.upload(h_x_, s)); SK_HIP_TRY(upload_padded(consts_, p.consts, s)); SK_HIP_TRY(upload_padded(const_off_, p.rb_const_off, s));
  SK_HIP_TRY(pidx_off_.upload(p.rb_pidx_off, s)); SK_HIP_TRY(upload_padded(xoff_, h_xoff_, s));
  SK_HIP_TRY(upload_padded(blocks_, P.blocks, s)); SK_HIP_TRY(upload_padded(members_, h_members_, s));
  SK_HIP_TRY(upload_padded(blk_stage_, P.blk_stage, s)); SK_HIP_TRY(upload_padded(blk_stride_, P.blk_stride, s));
  SK_HIP_TRY(blk_dim_.upload(h_blk_dim_, s)); SK_HIP_TRY(blk_loss_.upload(h_blk_loss_, s));
  SK_HIP_TRY(row_off_.upload(P.row_off, s)); SK_HIP_TRY(val_off_.upload(P.val_off, s)); SK_HIP_TRY(slot_begin_.upload(P.slot_begin, s));
  SK_HIP_TRY(upload_padded(slot_block_, P.slot_block, s)); SK_HIP_TRY(upload_padded(slot_k0_, P.slot_k0, s)); SK_HIP_TRY(upload_padded(slot_pos_, P.slot_pos, s));
  if (by_column) SK_HIP_TRY(upload_padded(slot_owner_, P.slot_owner, s));
  SK_HIP_TRY(pblocks_.upload(h_pblocks_, s)); SK_HIP_TRY(nodes_.upload(h_nodes_, s));
  SK_HIP_TRY(stage_.alloc(std::max<size_t>(P.stage_size, 1)));
  if (want_values) SK_HIP_TRY(values_.alloc((size_t)std::max<long long>(P.num_nonzeros, 1)));
  SK_HIP_TRY(fail_.alloc(1)); SK_HIP_TRY(fail_.zero(s));
  return SK_OK;
}

int DeviceJacobian::tape(int functor, const TapeDevBuffers** tb) {
  const bool fresh = tapes_.count(functor) == 0;
  TapeDevBuffers& t = tapes_[functor];
  if (fresh) SK_HIP_TRY(t.upload(*p_->tapes[functor - kTapeFunctorBase], s_));
  *tb = &t;
  return SK_OK;
}

int DeviceJacobian::upload_tapes() {
  const TapeDevBuffers* tb = nullptr;
  for (const EvaluateGroup& G : P_->groups)
    if (G.functor >= kTapeFunctorBase) { const int rc = tape(G.functor, &tb); if (rc != SK_OK) return rc; }
  return SK_OK;
}

int DeviceJacobian::evaluate(const double* x_dev, bool jac, const std::vector<size_t>* group_stage) {
  const Problem& p = *p_;
  const EvaluatePlan& P = *P_;
  EvaluateEvalArgs ea;
  ea.blocks = blocks_.p; ea.consts = consts_.p; ea.const_off = const_off_.p; ea.xoff = xoff_.p; ea.pidx_off = pidx_off_.p; ea.x = x_dev; ea.fail_flag = fail_.p;
  std::fill(h_cb_stage_.begin(), h_cb_stage_.end(), 0.0);
  for (size_t g = 0; g < P.groups.size(); ++g) {
    const EvaluateGroup& G = P.groups[g];
    if (G.functor == SK_FUNCTOR_HOST_CALLBACK) {  // the director path: the caller's Evaluate on the host, its rows uploaded below
      if (group_stage) { set_error("host-evaluated residual blocks have no staging but the plan's"); return SK_ERR_UNSUPPORTED; }
      const int b = P.blocks[G.members[0]];
      const CostFunction* cf = p.rb_cost[b];
      const int nblk = (int)cf->block_sizes.size(), nres = cf->num_residuals;
      std::vector<const double*> params(nblk);
      std::vector<std::vector<double>> jbuf(nblk);
      std::vector<double*> jptr(nblk);
      for (int q = 0; q < nblk; ++q) {
        params[q] = &h_x_[h_block_off_[p.rb_pidx[p.rb_pidx_off[b] + q]]];
        if (jac) jbuf[q].assign((size_t)nres * cf->block_sizes[q], 0.0);
        jptr[q] = jac ? jbuf[q].data() : nullptr;
      }
      double* out = &h_cb_stage_[G.stage_off - P.callback_stage_begin];  // (a group of one lane: the planes are the entries themselves)
      if (!cf->callback(cf->user, params.data(), out, jac ? jptr.data() : nullptr)) {
        set_error("Evaluate: the cost function of residual block %d reported failure", b);
        return SK_ERR_EVALUATION_FAILED;
      }
      if (jac) {
        int k0 = 0;
        for (int q = 0; q < nblk; ++q) {
          const int nq = cf->block_sizes[q];
          for (int r = 0; r < nres; ++r) for (int j = 0; j < nq; ++j) out[nres + r * G.dim + k0 + j] = jbuf[q][(size_t)r * nq + j];
          k0 += nq;
        }
      }
      continue;
    }
    ea.count = (int)G.members.size(); ea.members = members_.p + member_off_[g];
    ea.stage = stage_.p + (group_stage ? (*group_stage)[g] : G.stage_off);
    if (G.functor >= kTapeFunctorBase) {
      const TapeDevBuffers* tb = nullptr;
      const int rc = tape(G.functor, &tb);
      if (rc != SK_OK) return rc;
      if (!launch_evaluate_eval_tape(*tb, jac, ea, s_)) {
        set_error("a recorded functor needs %d registers: more than the device interpreter holds", p.tapes[G.functor - kTapeFunctorBase]->num_registers);
        return SK_ERR_UNSUPPORTED;
      }
    } else {
      launch_evaluate_eval(G.functor, jac, ea, s_);
    }
  }
  if (!h_cb_stage_.empty())
    SK_HIP_TRY(hipMemcpyAsync(stage_.p + P.callback_stage_begin, h_cb_stage_.data(), h_cb_stage_.size() * sizeof(double), hipMemcpyHostToDevice, s_));
  return SK_OK;
}

void DeviceJacobian::finish(const double* x_dev, double* residuals, double* values, double* cterm, const size_t* blk_stage) {
  EvaluateFinishArgs fa;
  fa.num_blocks = (int)P_->blocks.size(); fa.blk_stage = blk_stage ? blk_stage : blk_stage_.p; fa.blk_stride = blk_stride_.p; fa.blk_dim = blk_dim_.p; fa.blk_loss = blk_loss_.p;
  fa.row_off = row_off_.p; fa.val_off = val_off_.p; fa.slot_begin = slot_begin_.p; fa.slot_block = slot_block_.p; fa.slot_k0 = slot_k0_.p;
  fa.slot_pos = slot_pos_.p; fa.pblocks = pblocks_.p; fa.nodes = nodes_.p; fa.x = x_dev; fa.stage = stage_.p;
  fa.residuals = residuals; fa.values = values; fa.cterm = cterm;
  launch_evaluate_finish(fa, s_);
}

}  // namespace sk
