// sk_cholesky_solve* on the device: the fronts of chol_fronts.hpp uploaded, factored and solved by the plans of chol_kernels.hpp,
// their solutions scattered into x.  Everything of a call runs on the call's own stream, never the null stream: a null-stream copy
// would wait for every blocking stream of the device — among them a live solver's resident potrf server.
#include "chol_solve.hpp"

#include <memory>

#include "chol_fronts.hpp"
#include "chol_kernels.hpp"
#include "common.hpp"

namespace sk {
namespace {

// What every shape begins and ends with.  Declared before a call's device buffers: the stream outlives them on every path.
struct SolveDevice {
  CholeskyContext ctx;  // exercise the look-ahead path the solver uses
  StreamGuard stream;
  bool la = false;
  // prepare: the device's queue choice first (a second context takes the queues it leaves over)
  int open(bool prepare) {
    if (sk_device_count() <= 0) { set_error("no HIP device available: libskeres_amd has no CPU fallback"); return SK_ERR_NO_DEVICE; }
    SK_HIP_TRY(cholesky_init());
    la = ctx.init() == hipSuccess;
    if (!la) (void)hipGetLastError();
    SK_HIP_TRY(hipStreamCreateWithFlags(&stream.s, hipStreamNonBlocking));
    if (prepare && la) cholesky_prepare(&ctx, stream.s);
    return SK_OK;
  }
  CholeskyContext* context() { return la ? &ctx : nullptr; }
  bool chain(int automatic_plan) const { return automatic_plan != 0 && la && ctx.server != nullptr; }  // (the plan; resident or not is the device's state)
  // waits for the stream; what the factorisations and back-substitutions left in *dinfo decides
  int close(const int* dinfo) {
    int info = 0;
    SK_HIP_TRY(hipMemcpyAsync(&info, dinfo, sizeof(int), hipMemcpyDeviceToHost, stream.s));
    SK_HIP_TRY(hipStreamSynchronize(stream.s));
    if (info == 2) { (void)cholesky_note_info(&ctx, info); set_error("the resident panel chain timed out"); return SK_ERR_HIP; }
    if (info) { set_error("matrix is not positive definite"); return SK_ERR_EVALUATION_FAILED; }
    return SK_OK;
  }
};

int group_or_automatic(int group, int automatic_plan) { return group > 0 ? group : automatic_plan ? 1 : 3; }

hipError_t download(std::vector<double>& h, const double* d, hipStream_t s) { return hipMemcpyAsync(h.data(), d, h.size() * sizeof(double), hipMemcpyDeviceToHost, s); }

const int* envelope_of(const std::vector<int>& last) { return last.empty() ? nullptr : last.data(); }

}  // namespace

int cholesky_solve_single(int n, const double* A, const double* b, double* x, double* L, int group, const int* last, int automatic_plan, int border_begin_row) {
  if (last) {
    const int c = invalid_envelope_column(n, last);
    if (c >= 0) { set_error("invalid block envelope at block column %d", c); return SK_ERR_INVALID_ARGUMENT; }
  }
  SolveDevice dev;
  if (const int rc = dev.open(false)) return rc;
  hipStream_t s = dev.stream.s;
  group = group_or_automatic(group, automatic_plan);
  SingleFront f = single_front(n, A, b, border_begin_row);
  const int npad = f.npad;
  const int* tail = nullptr;
  if (border_begin_row >= 0) { last = f.last.data(); tail = f.tail.data(); }
  DevBuf<double> dS, dLinv, dw, dy; DevBuf<int> dinfo;
  SK_HIP_TRY(dS.upload(f.S, s)); SK_HIP_TRY(dLinv.alloc((size_t)npad * 128)); SK_HIP_TRY(dLinv.zero(s));
  SK_HIP_TRY(dy.alloc(npad)); SK_HIP_TRY(dw.alloc(npad)); SK_HIP_TRY(dinfo.alloc(1)); SK_HIP_TRY(dinfo.zero(s));
  cholesky_factor(dS.p, npad, npad, dLinv.p, dinfo.p, group, s, dev.context(), nullptr, last, dev.chain(automatic_plan), -1, 1, nullptr, tail);
  cholesky_backsolve(dS.p, npad, n, npad, f.rhs_row, dLinv.p, dw.p, dy.p, s, nullptr, last, dinfo.p, tail);
  if (const int rc = dev.close(dinfo.p)) return rc;
  std::vector<double> y(npad);
  SK_HIP_TRY(download(y, dy.p, s));
  if (L) SK_HIP_TRY(download(f.S, dS.p, s));
  SK_HIP_TRY(hipStreamSynchronize(s));
  single_front_solution(f, y, x);
  if (L) single_front_factor(f, f.S, L);
  return SK_OK;
}

int cholesky_solve_two_way(int n, const double* A, const double* b, double* x, int head, int tail_begin, int group, int automatic_plan) {
  const std::string why = two_way_check(n, A, head, tail_begin);
  if (!why.empty()) { set_error("%s", why.c_str()); return SK_ERR_INVALID_ARGUMENT; }
  SolveDevice dev;
  if (const int rc = dev.open(true)) return rc;
  hipStream_t s = dev.stream.s;
  CholeskyContext ctxB;
  const bool side = dev.la && ctxB.init_secondary(dev.ctx) == hipSuccess;
  if (dev.la && !side) (void)hipGetLastError();
  group = group_or_automatic(group, automatic_plan);
  const TwoWayFronts f = two_way_fronts(n, A, b, head, tail_begin);
  const size_t dA = f.A.dim, dB = f.B.dim, dR = f.R.dim;
  DevBuf<double> dFA, dFB, dFR, dLinv, dw, dy; DevBuf<int> dinfo, dmap;
  SK_HIP_TRY(dFA.upload(f.A.F, s)); SK_HIP_TRY(dFB.upload(f.B.F, s)); SK_HIP_TRY(dFR.upload(f.R.F, s)); SK_HIP_TRY(dmap.upload(f.mapB, s));
  SK_HIP_TRY(dLinv.alloc((size_t)(f.A.ncols + f.B.ncols + f.R.ncols) * 128 * 128)); SK_HIP_TRY(dLinv.zero(s));
  SK_HIP_TRY(dw.alloc(dA + dB + 2 * dR)); SK_HIP_TRY(dy.alloc(dA + dB + dR)); SK_HIP_TRY(dy.zero(s)); SK_HIP_TRY(dinfo.alloc(1)); SK_HIP_TRY(dinfo.zero(s));
  auto view = [](const HostFront& h, double* S, double* Linv) {
    FrontView v;
    v.S = S; v.ld = (long)h.dim; v.nblk = h.nblk; v.ncols = h.ncols; v.last = envelope_of(h.last); v.Linv = Linv; v.rhs_row = h.rhs_row;
    return v;
  };
  DissectedSystem d;
  d.A = view(f.A, dFA.p, dLinv.p);
  d.B = view(f.B, dFB.p, dLinv.p + (size_t)f.A.ncols * 128 * 128);
  d.R = view(f.R, dFR.p, dLinv.p + (size_t)(f.A.ncols + f.B.ncols) * 128 * 128);
  d.border_blocks = f.border_blocks; d.mapB = dmap.p;
  cholesky_dissected_factor(d, dinfo.p, group, s, dev.context(), side ? &ctxB : nullptr, nullptr, nullptr, dev.chain(automatic_plan));
  double *wA = dw.p, *wB = dw.p + dA, *wR = dw.p + dA + dB, *ybB = dw.p + dA + dB + dR;
  double *yA = dy.p, *yB = dy.p + dA, *yR = dy.p + dA + dB;
  cholesky_dissected_backsolve(d, f.sep_n, wR, yR, wA, yA, wB, yB, ybB, s, side ? &ctxB : nullptr, nullptr, dinfo.p);
  if (const int rc = dev.close(dinfo.p)) return rc;
  std::vector<double> y(dA + dB + dR);
  SK_HIP_TRY(download(y, dy.p, s));
  SK_HIP_TRY(hipStreamSynchronize(s));
  two_way_scatter(f, y.data(), x);
  return SK_OK;
}

int cholesky_solve_multi_way(int n, const double* A, const double* b, double* x, int num_segments, const int* cuts, int group, int automatic_plan) {
  const int R = num_segments;
  SegmentCuts c;
  const std::string why = segment_cuts(n, A, R, cuts, &c);
  if (!why.empty()) { set_error("%s", why.c_str()); return SK_ERR_INVALID_ARGUMENT; }
  SolveDevice dev;
  if (const int rc = dev.open(true)) return rc;
  hipStream_t s = dev.stream.s;
  group = group_or_automatic(group, automatic_plan);
  const bool chain = dev.chain(automatic_plan);
  const HostFront root = segments_root(c, A, b);
  const size_t dR = root.dim;
  const int* lastR = envelope_of(root.last);
  DevBuf<double> dFR; DevBuf<int> dinfo;
  SK_HIP_TRY(dFR.upload(root.F, s)); SK_HIP_TRY(dinfo.alloc(1)); SK_HIP_TRY(dinfo.zero(s));
  struct Leaf { LeafFront f; std::vector<double> yh; DevBuf<double> F, Linv, w, y, yb; DevBuf<int> dmap; };
  std::vector<std::unique_ptr<Leaf>> leaves;
  for (int k = 0; k < R; ++k) {
    std::unique_ptr<Leaf> lf(new Leaf());
    lf->f = segment_leaf(c, A, b, k);
    const SegmentLayout& L = lf->f.L;
    const size_t d = lf->f.dim, border = d - (size_t)L.ncols * 128;
    SK_HIP_TRY(lf->F.upload(lf->f.F, s)); SK_HIP_TRY(lf->dmap.upload(lf->f.map, s));
    SK_HIP_TRY(lf->Linv.alloc((size_t)L.ncols * 128 * 128)); SK_HIP_TRY(lf->Linv.zero(s));
    SK_HIP_TRY(lf->w.alloc(d)); SK_HIP_TRY(lf->y.alloc(d)); SK_HIP_TRY(lf->y.zero(s)); SK_HIP_TRY(lf->yb.alloc(border));
    if (lf->f.interior_n > 0) {
      cholesky_factor(lf->F.p, (long)d, (int)d, lf->Linv.p, dinfo.p, group, s, dev.context(), nullptr, lf->f.last.data(), chain, L.ncols, L.tail_rows);
      cholesky_border_add(dFR.p, (long)dR, lf->F.p, (long)d, L.ncols, L.nblk - L.ncols, lf->dmap.p, s);
    }
    SK_HIP_TRY(hipStreamSynchronize(s));
    std::vector<double>().swap(lf->f.F);  // (the host copy is on the device)
    leaves.push_back(std::move(lf));
  }
  DevBuf<double> dLinvR, dwR, dyR;
  SK_HIP_TRY(dLinvR.alloc(dR * 128)); SK_HIP_TRY(dLinvR.zero(s)); SK_HIP_TRY(dwR.alloc(dR)); SK_HIP_TRY(dyR.alloc(dR));
  cholesky_factor(dFR.p, (long)dR, (int)dR, dLinvR.p, dinfo.p, group, s, dev.context(), nullptr, lastR, chain);
  cholesky_backsolve(dFR.p, (long)dR, c.nroot, (int)dR, c.nroot, dLinvR.p, dwR.p, dyR.p, s, nullptr, lastR, dinfo.p);
  for (auto& lf : leaves) {
    const SegmentLayout& L = lf->f.L;
    if (L.ncols == 0) continue;
    const int m = (L.nblk - L.ncols) * 128;
    DevBuf<int> dg;
    SK_HIP_TRY(dg.upload(lf->f.gmap, s));
    cholesky_gather_map(dyR.p, dg.p, lf->yb.p, m, s);
    cholesky_backsolve_front(lf->F.p, (long)lf->f.dim, L.nblk, L.ncols, L.rhs_row, lf->Linv.p, lf->yb.p, lf->w.p, lf->y.p, s, lf->f.last.data(), L.spike, L.tail_rows, dinfo.p);
    SK_HIP_TRY(hipStreamSynchronize(s));  // (dg goes out of scope)
  }
  if (const int rc = dev.close(dinfo.p)) return rc;
  std::vector<double> yR(dR);
  SK_HIP_TRY(download(yR, dyR.p, s));
  for (auto& lf : leaves) { lf->yh.resize(lf->f.dim); SK_HIP_TRY(download(lf->yh, lf->y.p, s)); }
  SK_HIP_TRY(hipStreamSynchronize(s));
  segments_scatter_root(c, yR.data(), x);
  for (auto& lf : leaves) segments_scatter_leaf(lf->f, lf->yh.data(), x);
  return SK_OK;
}

}  // namespace sk
