// Problem::Evaluate on the device: the host side of sk_problem_evaluate.  Plan: evaluate_plan.cpp; kernels: evaluate_kernels.hip.
// One call = plan, its device image with the caller's parameter memory as it is now (jacobian_device.hpp), one evaluation launch
// per functor / tape (host-callback blocks through their sk_evaluate_fn, their staging uploaded), finish, gradient, cost, download
// what was asked for.
#include <algorithm>

#include "evaluate_kernels.hpp"
#include "evaluate_plan.hpp"
#include "jacobian_device.hpp"

namespace sk {

int problem_evaluate(const Problem& p, const EvaluateOptions* options, double* cost, double* residuals, double* gradient, double* values,
                     double* launch_seconds) {
  const bool want_jac = gradient || values;
  EvaluatePlan P;
  std::string why;
  int rc = evaluate_plan_build(p, options, false, gradient != nullptr, want_jac, &P, &why);
  if (rc != SK_OK) { set_error("%s", why.c_str()); return rc; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available: libskeres_amd has no CPU fallback"); return SK_ERR_NO_DEVICE; }
  if (!cost && !residuals && !gradient && !values) return SK_OK;
  if (options && options->device >= 0) SK_HIP_TRY(hipSetDevice(options->device));
  const bool apply_loss = !options || options->apply_loss_function;
  const int nb = (int)P.blocks.size();
  StreamGuard sg;  // (outlives the device buffers)
  DeviceJacobian J;
  J.gather(p, P, param_blocks(p, P, nullptr), apply_loss);

  SK_HIP_TRY(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
  hipStream_t s = sg.s;
  Marks marks; marks.on = launch_seconds != nullptr; marks.s = s;
  marks.mark();
  rc = J.upload(want_jac, /*by_column*/ gradient != nullptr, s);
  if (rc != SK_OK) return rc;
  DevBuf<double> d_res, d_cterm, d_partials, d_cost, d_grad;
  DevBuf<int> d_grad_col, d_grad_size, d_grad_begin, d_grad_slots;
  SK_HIP_TRY(d_res.alloc((size_t)std::max(P.num_rows, 1)));
  SK_HIP_TRY(d_cterm.alloc((size_t)std::max(nb, 1)));
  SK_HIP_TRY(d_partials.alloc((size_t)(nb / kEvaluateSumChunk + 1))); SK_HIP_TRY(d_cost.alloc(1));
  if (gradient) {
    SK_HIP_TRY(upload_padded(d_grad_col, P.grad_col, s)); SK_HIP_TRY(upload_padded(d_grad_size, P.grad_size, s));
    SK_HIP_TRY(d_grad_begin.upload(P.grad_begin, s)); SK_HIP_TRY(upload_padded(d_grad_slots, P.grad_slots, s));
    SK_HIP_TRY(d_grad.alloc((size_t)std::max(P.num_cols, 1))); SK_HIP_TRY(d_grad.zero(s));
  }
  marks.mark();

  rc = J.evaluate(J.x(), want_jac);  // a launch per functor / tape
  if (rc != SK_OK) return rc;
  SK_HIP_TRY(hipGetLastError());
  marks.mark();

  J.finish(J.x(), d_res.p, J.values(), d_cterm.p);
  marks.mark();
  if (gradient) {
    EvaluateGradientArgs ga;
    ga.num_column_blocks = (int)P.grad_col.size(); ga.grad_col = d_grad_col.p; ga.grad_size = d_grad_size.p; ga.grad_begin = d_grad_begin.p;
    ga.grad_slots = d_grad_slots.p; ga.slot_owner = J.slot_owner(); ga.slot_pos = J.slot_pos(); ga.row_off = J.row_off(); ga.val_off = J.val_off();
    ga.residuals = d_res.p; ga.values = J.values(); ga.gradient = d_grad.p;
    launch_evaluate_gradient(ga, s);
  }
  marks.mark();
  if (cost) launch_evaluate_cost(d_cterm.p, nb, d_partials.p, d_cost.p, s);
  SK_HIP_TRY(hipGetLastError());
  marks.mark();

  int failed = 0;
  SK_HIP_TRY(hipMemcpyAsync(&failed, J.fail_flag(), sizeof(int), hipMemcpyDeviceToHost, s));
  if (cost) SK_HIP_TRY(hipMemcpyAsync(cost, d_cost.p, sizeof(double), hipMemcpyDeviceToHost, s));
  if (residuals && P.num_rows > 0) SK_HIP_TRY(hipMemcpyAsync(residuals, d_res.p, (size_t)P.num_rows * sizeof(double), hipMemcpyDeviceToHost, s));
  if (gradient && P.num_cols > 0) SK_HIP_TRY(hipMemcpyAsync(gradient, d_grad.p, (size_t)P.num_cols * sizeof(double), hipMemcpyDeviceToHost, s));
  if (values && P.num_nonzeros > 0) SK_HIP_TRY(hipMemcpyAsync(values, J.values(), (size_t)P.num_nonzeros * sizeof(double), hipMemcpyDeviceToHost, s));
  marks.mark();
  SK_HIP_TRY(hipStreamSynchronize(s));
  if (launch_seconds) for (int i = 0; i < kEvaluatePhases; ++i) launch_seconds[i] = marks.seconds(i);
  if (failed) { set_error("Evaluate: a cost functor reported failure"); return SK_ERR_EVALUATION_FAILED; }
  return SK_OK;
}

}  // namespace sk
