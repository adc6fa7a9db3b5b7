// Problem::Evaluate on the device: the host side of sk_problem_evaluate.  Plan: evaluate_plan.cpp; kernels: evaluate_kernels.hip.
// One call = gather the caller's parameter memory, upload the plan, one evaluation launch per functor / tape (host-callback blocks
// through their sk_evaluate_fn, their staging uploaded), finish, gradient, cost, download what was asked for.
#include <cstring>
#include <map>

#include "evaluate_kernels.hpp"
#include "evaluate_plan.hpp"

namespace sk {

namespace {
struct StreamGuard {
  hipStream_t s = nullptr;
  ~StreamGuard() { if (s) (void)hipStreamDestroy(s); }
};
// device time between marks on the stream (only when the caller asked for launch times)
struct Marks {
  bool on = false;
  hipStream_t s = nullptr;
  std::vector<hipEvent_t> ev;
  void mark() { if (!on) return; hipEvent_t e; if (hipEventCreate(&e) == hipSuccess) { (void)hipEventRecord(e, s); ev.push_back(e); } }
  ~Marks() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
};
}  // namespace

int problem_evaluate(const Problem& p, const EvaluateOptions* options, double* cost, double* residuals, double* gradient, double* values,
                     double* launch_seconds, DevBuf<double>* keep_values) {
  const bool want_jac = gradient || values || keep_values;
  EvaluatePlan P;
  std::string why;
  int rc = evaluate_plan_build(p, options, false, gradient != nullptr, want_jac, &P, &why);
  if (rc != SK_OK) { set_error("%s", why.c_str()); return rc; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available: libskeres_amd has no CPU fallback"); return SK_ERR_NO_DEVICE; }
  if (!cost && !residuals && !gradient && !values && !keep_values) return SK_OK;
  if (options && options->device >= 0) SK_HIP_TRY(hipSetDevice(options->device));
  const bool apply_loss = !options || options->apply_loss_function;
  const int nb = (int)P.blocks.size(), num_pb = (int)p.block_ptr.size();

  // the point: the caller's parameter memory, now
  std::vector<int> block_off(num_pb + 1, 0);
  for (int b = 0; b < num_pb; ++b) block_off[b + 1] = block_off[b] + p.block_size[b];
  std::vector<double> x((size_t)std::max(block_off[num_pb], 1), 0.0);
  for (int b = 0; b < num_pb; ++b) std::memcpy(&x[block_off[b]], p.block_ptr[b], p.block_size[b] * sizeof(double));
  std::vector<int> xoff(std::max<size_t>(p.rb_pidx.size(), 1), 0);
  for (size_t i = 0; i < p.rb_pidx.size(); ++i) xoff[i] = block_off[p.rb_pidx[i]];
  std::vector<ParamBlock> pblocks((size_t)std::max(num_pb, 1));
  for (int b = 0; b < num_pb; ++b) {
    ParamBlock& pb = pblocks[b];
    const int pz = b < (int)p.block_param.size() ? p.block_param[b] : -1;
    pb.type = pz >= 0 ? p.params[pz].type : kParamIdentity;
    pb.global_size = p.block_size[b]; pb.local_size = P.col_size[b];
    pb.constant_mask = pz >= 0 ? p.params[pz].constant_mask : 0u;
    pb.global_off = block_off[b]; pb.local_off = P.col_off[b];
  }
  std::vector<int> blk_dim(std::max(nb, 1), 0), blk_loss(std::max(nb, 1), -1), members;
  for (const EvaluateGroup& G : P.groups) for (int i : G.members) blk_dim[i] = G.dim;
  for (int i = 0; i < nb; ++i) blk_loss[i] = apply_loss ? p.rb_loss[P.blocks[i]] : -1;
  std::vector<size_t> member_off;
  for (const EvaluateGroup& G : P.groups) { member_off.push_back(members.size()); members.insert(members.end(), G.members.begin(), G.members.end()); }
  std::vector<double> consts = p.consts; if (consts.empty()) consts.push_back(0.0);
  std::vector<LossNode> nodes = p.loss_nodes;
  if (nodes.empty()) { LossNode t; t.type = kLossTrivial; t.f = t.g = -1; t.depth = 0; t.a = t.b = 0.0; nodes.push_back(t); }
  auto padded = [](std::vector<int> v) { if (v.empty()) v.push_back(0); return v; };

  StreamGuard sg;
  SK_HIP_TRY(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
  hipStream_t s = sg.s;
  Marks marks; marks.on = launch_seconds != nullptr; marks.s = s;
  marks.mark();
  DevBuf<double> d_x, d_consts, d_stage, d_res, d_val, d_cterm, d_partials, d_cost, d_grad;
  DevBuf<size_t> d_const_off, d_pidx_off, d_blk_stage;
  DevBuf<int> d_xoff, d_blocks, d_members, d_blk_stride, d_blk_dim, d_blk_loss, d_row_off, d_val_off, d_slot_begin, d_slot_block, d_slot_k0, d_slot_pos,
      d_slot_owner, d_grad_col, d_grad_size, d_grad_begin, d_grad_slots, d_fail;
  DevBuf<ParamBlock> d_pblocks;
  DevBuf<LossNode> d_nodes;
  SK_HIP_TRY(d_x.upload(x, s)); SK_HIP_TRY(d_consts.upload(consts, s));
  { std::vector<size_t> co = p.rb_const_off; if (co.empty()) co.push_back(0); SK_HIP_TRY(d_const_off.upload(co, s)); }
  SK_HIP_TRY(d_pidx_off.upload(p.rb_pidx_off, s)); SK_HIP_TRY(d_xoff.upload(xoff, s));
  SK_HIP_TRY(d_blocks.upload(padded(P.blocks), s)); SK_HIP_TRY(d_members.upload(padded(members), s));
  { std::vector<size_t> bs = P.blk_stage; if (bs.empty()) bs.push_back(0); SK_HIP_TRY(d_blk_stage.upload(bs, s)); }
  SK_HIP_TRY(d_blk_stride.upload(padded(P.blk_stride), s)); SK_HIP_TRY(d_blk_dim.upload(blk_dim, s)); SK_HIP_TRY(d_blk_loss.upload(blk_loss, s));
  SK_HIP_TRY(d_row_off.upload(P.row_off, s)); SK_HIP_TRY(d_val_off.upload(P.val_off, s)); SK_HIP_TRY(d_slot_begin.upload(P.slot_begin, s));
  SK_HIP_TRY(d_slot_block.upload(padded(P.slot_block), s)); SK_HIP_TRY(d_slot_k0.upload(padded(P.slot_k0), s)); SK_HIP_TRY(d_slot_pos.upload(padded(P.slot_pos), s));
  SK_HIP_TRY(d_pblocks.upload(pblocks, s)); SK_HIP_TRY(d_nodes.upload(nodes, s));
  SK_HIP_TRY(d_stage.alloc(std::max<size_t>(P.stage_size, 1)));
  SK_HIP_TRY(d_res.alloc((size_t)std::max(P.num_rows, 1)));
  if (want_jac) SK_HIP_TRY(d_val.alloc((size_t)std::max<long long>(P.num_nonzeros, 1)));
  SK_HIP_TRY(d_cterm.alloc((size_t)std::max(nb, 1)));
  SK_HIP_TRY(d_partials.alloc((size_t)(nb / kEvaluateSumChunk + 1))); SK_HIP_TRY(d_cost.alloc(1));
  SK_HIP_TRY(d_fail.alloc(1)); SK_HIP_TRY(d_fail.zero(s));
  if (gradient) {
    SK_HIP_TRY(d_slot_owner.upload(padded(P.slot_owner), s));
    SK_HIP_TRY(d_grad_col.upload(padded(P.grad_col), s)); SK_HIP_TRY(d_grad_size.upload(padded(P.grad_size), s));
    SK_HIP_TRY(d_grad_begin.upload(P.grad_begin, s)); SK_HIP_TRY(d_grad_slots.upload(padded(P.grad_slots), s));
    SK_HIP_TRY(d_grad.alloc((size_t)std::max(P.num_cols, 1))); SK_HIP_TRY(d_grad.zero(s));
  }
  marks.mark();

  // evaluation: a launch per functor / tape
  std::map<int, TapeDevBuffers> tapes_dev;
  EvaluateEvalArgs ea;
  ea.blocks = d_blocks.p; ea.consts = d_consts.p; ea.const_off = d_const_off.p; ea.xoff = d_xoff.p; ea.pidx_off = d_pidx_off.p; ea.x = d_x.p; ea.fail_flag = d_fail.p;
  std::vector<double> cb_stage(P.stage_size - P.callback_stage_begin, 0.0);
  for (size_t g = 0; g < P.groups.size(); ++g) {
    const EvaluateGroup& G = P.groups[g];
    if (G.functor == SK_FUNCTOR_HOST_CALLBACK) {  // the director path: the caller's Evaluate on the host, its rows uploaded below
      const int b = P.blocks[G.members[0]];
      const CostFunction* cf = p.rb_cost[b];
      const int nblk = (int)cf->block_sizes.size(), nres = cf->num_residuals;
      std::vector<const double*> params(nblk);
      std::vector<std::vector<double>> jbuf(nblk);
      std::vector<double*> jptr(nblk);
      for (int q = 0; q < nblk; ++q) {
        params[q] = &x[block_off[p.rb_pidx[p.rb_pidx_off[b] + q]]];
        if (want_jac) jbuf[q].assign((size_t)nres * cf->block_sizes[q], 0.0);
        jptr[q] = want_jac ? jbuf[q].data() : nullptr;
      }
      double* out = &cb_stage[G.stage_off - P.callback_stage_begin];  // (a group of one lane: the planes are the entries themselves)
      if (!cf->callback(cf->user, params.data(), out, want_jac ? jptr.data() : nullptr)) {
        set_error("Evaluate: the cost function of residual block %d reported failure", b);
        return SK_ERR_EVALUATION_FAILED;
      }
      if (want_jac) {
        int k0 = 0;
        for (int q = 0; q < nblk; ++q) {
          const int nq = cf->block_sizes[q];
          for (int r = 0; r < nres; ++r) for (int j = 0; j < nq; ++j) out[nres + r * G.dim + k0 + j] = jbuf[q][(size_t)r * nq + j];
          k0 += nq;
        }
      }
      continue;
    }
    ea.count = (int)G.members.size(); ea.members = d_members.p + member_off[g]; ea.stage = d_stage.p + G.stage_off;
    if (G.functor >= kTapeFunctorBase) {
      const Tape& t = *p.tapes[G.functor - kTapeFunctorBase];
      TapeDevBuffers& tb = tapes_dev[G.functor];
      SK_HIP_TRY(tb.upload(t, s));
      if (!launch_evaluate_eval_tape(tb, want_jac, ea, s)) {
        set_error("a recorded functor needs %d registers: more than the device interpreter holds", t.num_registers);
        return SK_ERR_UNSUPPORTED;
      }
    } else {
      launch_evaluate_eval(G.functor, want_jac, ea, s);
    }
  }
  if (!cb_stage.empty()) SK_HIP_TRY(hipMemcpyAsync(d_stage.p + P.callback_stage_begin, cb_stage.data(), cb_stage.size() * sizeof(double), hipMemcpyHostToDevice, s));
  SK_HIP_TRY(hipGetLastError());
  marks.mark();

  EvaluateFinishArgs fa;
  fa.num_blocks = nb; fa.blk_stage = d_blk_stage.p; fa.blk_stride = d_blk_stride.p; fa.blk_dim = d_blk_dim.p; fa.blk_loss = d_blk_loss.p;
  fa.row_off = d_row_off.p; fa.val_off = d_val_off.p; fa.slot_begin = d_slot_begin.p; fa.slot_block = d_slot_block.p; fa.slot_k0 = d_slot_k0.p;
  fa.slot_pos = d_slot_pos.p; fa.pblocks = d_pblocks.p; fa.nodes = d_nodes.p; fa.x = d_x.p; fa.stage = d_stage.p;
  fa.residuals = d_res.p; fa.values = want_jac ? d_val.p : nullptr; fa.cterm = d_cterm.p;
  launch_evaluate_finish(fa, s);
  marks.mark();
  if (gradient) {
    EvaluateGradientArgs ga;
    ga.num_column_blocks = (int)P.grad_col.size(); ga.grad_col = d_grad_col.p; ga.grad_size = d_grad_size.p; ga.grad_begin = d_grad_begin.p;
    ga.grad_slots = d_grad_slots.p; ga.slot_owner = d_slot_owner.p; ga.slot_pos = d_slot_pos.p; ga.row_off = d_row_off.p; ga.val_off = d_val_off.p;
    ga.residuals = d_res.p; ga.values = d_val.p; ga.gradient = d_grad.p;
    launch_evaluate_gradient(ga, s);
  }
  marks.mark();
  if (cost) launch_evaluate_cost(d_cterm.p, nb, d_partials.p, d_cost.p, s);
  SK_HIP_TRY(hipGetLastError());
  marks.mark();

  int failed = 0;
  SK_HIP_TRY(hipMemcpyAsync(&failed, d_fail.p, sizeof(int), hipMemcpyDeviceToHost, s));
  if (cost) SK_HIP_TRY(hipMemcpyAsync(cost, d_cost.p, sizeof(double), hipMemcpyDeviceToHost, s));
  if (residuals && P.num_rows > 0) SK_HIP_TRY(hipMemcpyAsync(residuals, d_res.p, (size_t)P.num_rows * sizeof(double), hipMemcpyDeviceToHost, s));
  if (gradient && P.num_cols > 0) SK_HIP_TRY(hipMemcpyAsync(gradient, d_grad.p, (size_t)P.num_cols * sizeof(double), hipMemcpyDeviceToHost, s));
  if (values && P.num_nonzeros > 0) SK_HIP_TRY(hipMemcpyAsync(values, d_val.p, (size_t)P.num_nonzeros * sizeof(double), hipMemcpyDeviceToHost, s));
  marks.mark();
  SK_HIP_TRY(hipStreamSynchronize(s));
  if (launch_seconds) {
    for (int i = 0; i < kEvaluatePhases; ++i) {
      float ms = 0.f;
      launch_seconds[i] = (size_t)i + 1 < marks.ev.size() && hipEventElapsedTime(&ms, marks.ev[i], marks.ev[i + 1]) == hipSuccess ? 1e-3 * ms : 0.0;
    }
  }
  if (failed) { set_error("Evaluate: a cost functor reported failure"); return SK_ERR_EVALUATION_FAILED; }
  if (keep_values) { keep_values->release(); keep_values->p = d_val.p; keep_values->n = d_val.n; d_val.p = nullptr; d_val.n = 0; }  // (the caller's from here on)
  return SK_OK;
}

}  // namespace sk
