// ceres::Covariance on the device: the host side of sk_covariance_compute.  Plan: covariance_plan.cpp; kernels: covariance_kernels.hip.
// One compute = Problem::Evaluate's launches (its values array stays on the device), H = J^T J assembled dense (lower triangle),
// H~ = D H D with the k selected columns as unit rows behind it, a PARTIAL factorisation of the bordered matrix by cholesky_factor
// — H's block columns are factored, the border is left holding -Sel^T H~^-1 Sel, the selected block of the inverse, negated —,
// the pivot ratio, the extraction of the requested blocks into one packed buffer, one download.  Everything runs on one stream,
// launch by launch: no resident chain, no kernel that waits for another.  With CovarianceOptions::schur_elimination an independent
// set of column blocks is eliminated block by block in front of that factorisation and substituted back behind it (covariance_plan.hpp,
// "Schur elimination"): the dense matrix is then the reduced one, S~ = U~ - sum_e X_ge X_g'e^T.
#include <algorithm>
#include <climits>
#include <cmath>

#include "chol_kernels.hpp"
#include "covariance.hpp"
#include "covariance_kernels.hpp"
#include "covariance_plan.hpp"
#include "evaluate_kernels.hpp"
#include "jacobian_device.hpp"

namespace sk {

namespace {
constexpr int kCovarianceGroup = 3;  // SYRK depth of a full factorisation in 128-column blocks (Options::cholesky_group's automatic choice)

// The bordered matrix of steps 3 to 5: H (n columns, padded to npad_h) and the k border rows behind it.
struct Bordered {
  int n = 0, npad_h = 0, k = 0, npad = 0;
  long ld = 0;
  DevBuf<double> S, Linv, d, ratio;
  DevBuf<int> zero_col, info, sel_col;
  double* border() const { return S.p + (long)npad_h * ld + npad_h; }
  // S zeroed (the assembly stores every structural non-zero of the lower triangle once)
  int alloc(int n_, const std::vector<int>& sel, hipStream_t s) {
    n = n_; k = (int)sel.size();
    npad_h = std::max(1, (n + 127) / 128) * 128;
    npad = npad_h + std::max(1, (k + 127) / 128) * 128;
    ld = npad;
    SK_HIP_TRY(S.alloc((size_t)npad * npad)); SK_HIP_TRY(S.zero(s));
    SK_HIP_TRY(Linv.alloc((size_t)npad_h * 128)); SK_HIP_TRY(Linv.zero(s));
    SK_HIP_TRY(d.alloc((size_t)npad_h)); SK_HIP_TRY(ratio.alloc(2)); SK_HIP_TRY(ratio.zero(s));
    SK_HIP_TRY(info.alloc(1)); SK_HIP_TRY(info.zero(s));
    const std::vector<int> none(1, INT_MAX);
    SK_HIP_TRY(zero_col.upload(none, s));
    SK_HIP_TRY(upload_padded(sel_col, sel, s));
    SK_HIP_TRY(hipStreamSynchronize(s));  // (`none` goes out of scope)
    return SK_OK;
  }
  // step 3; *zero: the first column with an exactly zero diagonal entry (INT_MAX: none)
  int scale(hipStream_t s, int* zero, Marks* marks) {
    launch_cov_scale(S.p, ld, n, npad_h, d.p, zero_col.p, sel_col.p, k, s);
    SK_HIP_TRY(hipGetLastError());
    if (marks) marks->mark();
    SK_HIP_TRY(hipMemcpyAsync(zero, zero_col.p, sizeof(int), hipMemcpyDeviceToHost, s));
    SK_HIP_TRY(hipStreamSynchronize(s));
    return SK_OK;
  }
  // steps 4 and 5
  int factor(hipStream_t s, Marks* marks) {
    SK_HIP_TRY(cholesky_init());
    cholesky_factor(S.p, ld, npad, Linv.p, info.p, kCovarianceGroup, s, /*ctx*/ nullptr, /*kt*/ nullptr, /*last*/ nullptr, /*allow_chain*/ false,
                    /*ncols*/ npad_h / 128, /*tail_rows*/ (npad - npad_h) / 128);
    launch_cov_pivot_ratio(S.p, ld, n, ratio.p, s);
    SK_HIP_TRY(hipGetLastError());
    if (marks) marks->mark();
    return SK_OK;
  }
  // steps 3 to 5 (a zero diagonal entry: the matrix is not factored)
  int scale_and_factor(hipStream_t s, int* zero, Marks* marks) {
    const int rc = scale(s, zero, marks);
    return rc != SK_OK || *zero != INT_MAX ? rc : factor(s, marks);
  }
};
}  // namespace

int Covariance::compute(const Problem& p, double* const* blocks1, double* const* blocks2, int num_pairs) {
  valid_ = false; has_stats_ = false;
  if (num_pairs <= 0 || !blocks1 || !blocks2) { set_error("Covariance: no covariance blocks were asked for"); return SK_ERR_INVALID_ARGUMENT; }
  std::vector<std::pair<int, int>> pairs;
  for (int i = 0; i < num_pairs; ++i) {
    auto a = p.block_of.find(blocks1[i]), b = p.block_of.find(blocks2[i]);
    if (a == p.block_of.end() || b == p.block_of.end()) {
      set_error("Covariance: block %d of pair %d is no parameter block of the problem", a == p.block_of.end() ? 1 : 2, i);
      return SK_ERR_INVALID_ARGUMENT;
    }
    pairs.emplace_back(a->second, b->second);
  }
  return run(p, pairs);
}

int Covariance::run(const Problem& p, const std::vector<std::pair<int, int>>& pairs) {
  CovariancePlan C;
  std::string why;
  const bool schur = opt_.schur_elimination;
  int rc = covariance_plan_build(p, pairs, &C, &why, schur);
  if (rc != SK_OK) { set_error("%s", why.c_str()); return rc; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available: libskeres_amd has no CPU fallback"); return SK_ERR_NO_DEVICE; }
  if (opt_.device >= 0) SK_HIP_TRY(hipSetDevice(opt_.device));
  const EvaluatePlan& E = C.eval;
  const TangentColumns& T = C.cols;
  const PartList& parts = C.pair_parts;
  const PartList& sparts = C.schur_parts;
  const int num_pb = (int)p.block_ptr.size(), N = T.num_cols;

  // step 1: the evaluation, by Problem::Evaluate's own code (jacobian_device.hpp); the values array, the point (for the
  // Plus-Jacobians of the lift) and the parameter blocks stay on the device, where the assembly and the extraction read them
  StreamGuard sg;
  SK_HIP_TRY(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
  hipStream_t s = sg.s;
  DeviceJacobian dj;
  dj.gather(p, E, param_blocks(p, E, &T), opt_.apply_loss_function);
  rc = dj.upload(/*want_values*/ true, /*by_column*/ true, s);
  if (rc != SK_OK) return rc;
  DevBuf<double> d_res, d_cterm;
  SK_HIP_TRY(d_res.alloc((size_t)std::max(E.num_rows, 1))); SK_HIP_TRY(d_cterm.alloc(std::max<size_t>(E.blocks.size(), 1)));
  Marks eval_marks; eval_marks.s = s;
  eval_marks.mark();
  rc = dj.evaluate(dj.x(), true);
  if (rc != SK_OK) return rc;
  SK_HIP_TRY(hipGetLastError());
  dj.finish(dj.x(), d_res.p, dj.values(), d_cterm.p);
  eval_marks.mark();
  int failed = 0;
  SK_HIP_TRY(hipMemcpyAsync(&failed, dj.fail_flag(), sizeof(int), hipMemcpyDeviceToHost, s));

  DevBuf<int> d_part_pair, d_part_begin, d_part_end, d_part_out, d_long_pair, d_long_begin, d_pair_i, d_pair_j, d_term_si, d_term_sj, d_cb_col, d_cb_size, d_ra, d_rb,
      d_a, d_b;
  DevBuf<long> d_tan_off, d_amb_off;
  DevBuf<double> d_partial, d_out;
  SK_HIP_TRY(upload_padded(d_part_pair, parts.owner, s)); SK_HIP_TRY(upload_padded(d_part_begin, parts.begin, s));
  SK_HIP_TRY(upload_padded(d_part_end, parts.end, s)); SK_HIP_TRY(upload_padded(d_part_out, parts.out, s));
  SK_HIP_TRY(upload_padded(d_long_pair, parts.long_owner, s)); SK_HIP_TRY(d_long_begin.upload(parts.long_begin, s));
  SK_HIP_TRY(upload_padded(d_pair_i, C.pair_i, s)); SK_HIP_TRY(upload_padded(d_pair_j, C.pair_j, s));
  SK_HIP_TRY(upload_padded(d_term_si, C.term_si, s)); SK_HIP_TRY(upload_padded(d_term_sj, C.term_sj, s));
  SK_HIP_TRY(upload_padded(d_cb_col, T.cb_col, s)); SK_HIP_TRY(upload_padded(d_cb_size, T.cb_size, s));
  SK_HIP_TRY(upload_padded(d_ra, C.req_ra, s)); SK_HIP_TRY(upload_padded(d_rb, C.req_rb, s));
  SK_HIP_TRY(upload_padded(d_a, C.req_a, s)); SK_HIP_TRY(upload_padded(d_b, C.req_b, s));
  SK_HIP_TRY(upload_padded(d_tan_off, C.req_tan_off, s)); SK_HIP_TRY(upload_padded(d_amb_off, C.req_amb_off, s));
  SK_HIP_TRY(d_partial.alloc((size_t)std::max(parts.num_partials, 1) * kCovarianceTile));
  SK_HIP_TRY(d_out.alloc((size_t)std::max<long>(C.out_size, 1))); SK_HIP_TRY(d_out.zero(s));
  // Schur elimination: what the plan adds, the tiles, the diagonal over all columns, the pivots of the e-blocks
  DevBuf<int> d_cb_red, d_cb_elim, d_pair_tile, d_pair_flip, d_e_cb, d_ew_begin, d_ew_tile, d_ew_g, d_ew_sel, d_sp_i, d_sp_j, d_st_a, d_st_b, d_st_ne, d_spart_pair,
      d_spart_begin, d_spart_end, d_spart_out, d_slong_pair, d_slong_begin, d_req_ea, d_req_eb, d_zero, d_einfo;
  DevBuf<double> d_tiles, d_all, d_slot, d_spartial;
  const std::vector<int> no_zero(1, INT_MAX);
  if (schur) {
    SK_HIP_TRY(upload_padded(d_cb_red, C.cb_red, s)); SK_HIP_TRY(upload_padded(d_cb_elim, C.cb_elim, s));
    SK_HIP_TRY(upload_padded(d_pair_tile, C.pair_tile, s)); SK_HIP_TRY(upload_padded(d_pair_flip, C.pair_flip, s));
    SK_HIP_TRY(upload_padded(d_e_cb, C.e_cb, s)); SK_HIP_TRY(d_ew_begin.upload(C.ew_begin, s));
    SK_HIP_TRY(upload_padded(d_ew_tile, C.ew_tile, s)); SK_HIP_TRY(upload_padded(d_ew_g, C.ew_g, s)); SK_HIP_TRY(upload_padded(d_ew_sel, C.ew_sel, s));
    SK_HIP_TRY(upload_padded(d_sp_i, C.sp_i, s)); SK_HIP_TRY(upload_padded(d_sp_j, C.sp_j, s));
    SK_HIP_TRY(upload_padded(d_st_a, C.st_a, s)); SK_HIP_TRY(upload_padded(d_st_b, C.st_b, s)); SK_HIP_TRY(upload_padded(d_st_ne, C.st_ne, s));
    SK_HIP_TRY(upload_padded(d_spart_pair, sparts.owner, s)); SK_HIP_TRY(upload_padded(d_spart_begin, sparts.begin, s));
    SK_HIP_TRY(upload_padded(d_spart_end, sparts.end, s)); SK_HIP_TRY(upload_padded(d_spart_out, sparts.out, s));
    SK_HIP_TRY(upload_padded(d_slong_pair, sparts.long_owner, s)); SK_HIP_TRY(d_slong_begin.upload(sparts.long_begin, s));
    SK_HIP_TRY(upload_padded(d_req_ea, C.req_ea, s)); SK_HIP_TRY(upload_padded(d_req_eb, C.req_eb, s));
    SK_HIP_TRY(d_zero.upload(no_zero, s)); SK_HIP_TRY(d_einfo.alloc(1)); SK_HIP_TRY(d_einfo.zero(s));
    SK_HIP_TRY(d_tiles.alloc((size_t)std::max(C.num_tiles, 1) * kCovarianceTile)); SK_HIP_TRY(d_tiles.zero(s));  // (an e-block that no residual block names keeps a zero tile)
    SK_HIP_TRY(d_all.alloc((size_t)std::max(N, 1))); SK_HIP_TRY(d_slot.alloc((size_t)std::max(2 * C.num_elim, 1)));
    SK_HIP_TRY(d_spartial.alloc((size_t)std::max(sparts.num_partials, 1) * kCovarianceTile));
  }
  SK_HIP_TRY(hipStreamSynchronize(s));
  if (failed) { set_error("Evaluate: a cost functor reported failure"); return SK_ERR_EVALUATION_FAILED; }

  stats_.clear();
  stats_["columns"] = N; stats_["selected_columns"] = C.k; stats_["normal_matrix_pairs"] = (double)C.pair_i.size();
  stats_["reciprocal_pivot_ratio"] = 0.0;
  stats_["schur_elimination"] = schur ? 1 : 0; stats_["eliminated_blocks"] = C.num_elim; stats_["reduced_columns"] = schur ? C.red_cols : N;
  stats_["schur_terms"] = (double)C.schur_terms;
  double phase[kCovariancePhases] = {0, 0, 0, 0, 0};
  phase[0] = eval_marks.seconds(0);  // (the evaluation launches and the finish: what produces the values array)
  auto keep_stats = [&] {
    for (int i = 0; i < kCovariancePhases; ++i) stats_["phase_seconds_" + std::to_string(i)] = phase[i];
    has_stats_ = true;
  };

  Marks marks; marks.s = s;
  marks.mark();
  Bordered B;
  rc = B.alloc(schur ? C.red_cols : N, C.sel_col, s);
  if (rc != SK_OK) return rc;
  // step 2: the normal matrix
  CovJac J{dj.values(), dj.val_off(), dj.row_off(), dj.slot_owner(), dj.slot_pos()};
  CovPairs P;
  P.num_parts = (int)parts.owner.size(); P.num_long = (int)parts.long_owner.size();
  P.part_pair = d_part_pair.p; P.part_begin = d_part_begin.p; P.part_end = d_part_end.p; P.part_out = d_part_out.p;
  P.long_pair = d_long_pair.p; P.long_begin = d_long_begin.p; P.pair_i = d_pair_i.p; P.pair_j = d_pair_j.p;
  P.term_si = d_term_si.p; P.term_sj = d_term_sj.p; P.cb_col = d_cb_col.p; P.cb_size = d_cb_size.p;
  CovSchur Sc = {};
  if (schur) {  // the (f, f') pairs go to the reduced matrix, the others to their tiles
    P.cb_col = d_cb_red.p; P.pair_tile = d_pair_tile.p; P.pair_flip = d_pair_flip.p; P.tiles = d_tiles.p;
    Sc.num_cb = (int)T.cb_col.size(); Sc.num_e = C.num_elim;
    Sc.cb_col = d_cb_col.p; Sc.cb_red = d_cb_red.p; Sc.cb_size = d_cb_size.p; Sc.cb_elim = d_cb_elim.p; Sc.e_cb = d_e_cb.p;
    Sc.ew_begin = d_ew_begin.p; Sc.ew_tile = d_ew_tile.p; Sc.ew_g = d_ew_g.p; Sc.ew_sel = d_ew_sel.p; Sc.tiles = d_tiles.p;
    Sc.num_parts = (int)sparts.owner.size(); Sc.num_long = (int)sparts.long_owner.size();
    Sc.part_pair = d_spart_pair.p; Sc.part_begin = d_spart_begin.p; Sc.part_end = d_spart_end.p; Sc.part_out = d_spart_out.p;
    Sc.long_pair = d_slong_pair.p; Sc.long_begin = d_slong_begin.p; Sc.pair_i = d_sp_i.p; Sc.pair_j = d_sp_j.p;
    Sc.term_a = d_st_a.p; Sc.term_b = d_st_b.p; Sc.term_ne = d_st_ne.p; Sc.req_ea = d_req_ea.p; Sc.req_eb = d_req_eb.p;
  }
  launch_cov_normal_assemble(J, P, B.S.p, B.ld, d_partial.p, s);
  // steps 3 to 5
  int zero = INT_MAX;
  if (!schur) {
    rc = B.scale_and_factor(s, &zero, &marks);
    if (rc != SK_OK) return rc;
  } else {
    // d over all columns first: the e-blocks need it before U is scaled, and a zero entry ends the compute here
    launch_cov_schur_diag(Sc, B.S.p, B.ld, d_all.p, d_zero.p, s);
    SK_HIP_TRY(hipGetLastError());
    SK_HIP_TRY(hipMemcpyAsync(&zero, d_zero.p, sizeof(int), hipMemcpyDeviceToHost, s));
    SK_HIP_TRY(hipStreamSynchronize(s));
    if (zero == INT_MAX) {
      launch_cov_schur_eblocks(Sc, d_all.p, d_slot.p, d_einfo.p, s);
      int zero_f = INT_MAX;  // (no zero among the F columns: d_all covers them)
      rc = B.scale(s, &zero_f, nullptr);
      if (rc != SK_OK) return rc;
      launch_cov_schur_update(Sc, B.S.p, B.ld, d_spartial.p, s);
      SK_HIP_TRY(hipGetLastError());
      marks.mark();
      rc = B.factor(s, nullptr);
      if (rc != SK_OK) return rc;
      launch_cov_schur_pivot_ratio(d_slot.p, C.num_elim, B.ratio.p, s);
      SK_HIP_TRY(hipGetLastError());
      marks.mark();
    } else {
      marks.mark();
    }
  }
  if (zero != INT_MAX) {
    SK_HIP_TRY(hipStreamSynchronize(s));
    phase[1] = marks.seconds(0);
    int cb = 0;
    while (cb + 1 < (int)T.cb_col.size() && T.cb_col[cb + 1] <= zero) ++cb;
    keep_stats();
    set_error("Covariance: the Jacobian is rank deficient: column %d (parameter block %d, coordinate %d of its tangent space) is zero — no residual block depends on it",
              zero, T.cb_block[cb], zero - T.cb_col[cb]);
    return SK_ERR_EVALUATION_FAILED;
  }
  // step 6: the requested blocks, one packed buffer, one download
  CovRequests R;
  R.num = (int)C.req_a.size(); R.ra = d_ra.p; R.rb = d_rb.p; R.a = d_a.p; R.b = d_b.p; R.tan_off = d_tan_off.p; R.amb_off = d_amb_off.p;
  R.pblocks = dj.pblocks(); R.x = dj.x();
  if (schur) launch_cov_schur_extract(R, Sc, B.border(), B.ld, d_all.p, d_out.p, s);
  else launch_cov_extract(R, B.border(), B.ld, B.d.p, d_out.p, s);
  SK_HIP_TRY(hipGetLastError());
  marks.mark();
  std::vector<double> out((size_t)std::max<long>(C.out_size, 1));
  double ratio[2] = {0, 0};
  int info = 0, einfo = 0;
  if (schur) SK_HIP_TRY(hipMemcpyAsync(&einfo, d_einfo.p, sizeof(int), hipMemcpyDeviceToHost, s));
  SK_HIP_TRY(hipMemcpyAsync(out.data(), d_out.p, out.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  SK_HIP_TRY(hipMemcpyAsync(ratio, B.ratio.p, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
  SK_HIP_TRY(hipMemcpyAsync(&info, B.info.p, sizeof(int), hipMemcpyDeviceToHost, s));
  marks.mark();
  SK_HIP_TRY(hipStreamSynchronize(s));
  phase[1] = marks.seconds(0); phase[2] = marks.seconds(1); phase[3] = marks.seconds(2); phase[4] = marks.seconds(3);
  const double rcond = N == 0 ? 1.0 : ratio[1] > 0.0 && std::isfinite(ratio[0]) && std::isfinite(ratio[1]) ? ratio[0] / ratio[1] : 0.0;  // (N == 0: every block is constant)
  stats_["reciprocal_pivot_ratio"] = rcond;
  keep_stats();
  if (info != 0 || einfo != 0 || (N > 0 && (!(ratio[0] > 0.0) || !std::isfinite(ratio[1])))) {
    set_error("Covariance: the Jacobian is rank deficient: the factorisation of J^T J met a pivot that is not positive");
    return SK_ERR_EVALUATION_FAILED;
  }
  if (rcond < opt_.min_reciprocal_condition_number) {
    set_error("Covariance: the Jacobian is rank deficient: pivot ratio min L_jj^2 / max L_jj^2 = %.3e of the scaled normal matrix is below min_reciprocal_condition_number = %.3e",
              rcond, opt_.min_reciprocal_condition_number);
    return SK_ERR_EVALUATION_FAILED;
  }

  block_of_.clear();
  for (int b = 0; b < num_pb; ++b) block_of_[p.block_ptr[b]] = b;
  size_ = T.pb_size; tangent_ = T.pb_local_size;
  req_of_.clear();
  for (size_t r = 0; r < C.req_a.size(); ++r) req_of_[{C.req_a[r], C.req_b[r]}] = (int)r;
  tan_off_ = C.req_tan_off; amb_off_ = C.req_amb_off;
  out_.swap(out);
  valid_ = true;
  return SK_OK;
}

int Covariance::get_block(const double* b1, const double* b2, bool tangent, double* out) const {
  if (!valid_) { set_error("Covariance: no covariance has been computed (call compute first; a failed compute leaves none)"); return SK_ERR_INVALID_ARGUMENT; }
  if (!out) { set_error("null argument"); return SK_ERR_INVALID_ARGUMENT; }
  auto a = block_of_.find(b1), b = block_of_.find(b2);
  if (a == block_of_.end() || b == block_of_.end()) { set_error("Covariance: not a parameter block of the problem the covariance was computed for"); return SK_ERR_INVALID_ARGUMENT; }
  const int ia = a->second, ib = b->second;
  auto r = req_of_.find({std::min(ia, ib), std::max(ia, ib)});
  if (r == req_of_.end()) { set_error("Covariance: the covariance of parameter blocks %d and %d was not computed", ia, ib); return SK_ERR_INVALID_ARGUMENT; }
  const std::vector<int>& sz = tangent ? tangent_ : size_;
  const double* src = out_.data() + (tangent ? tan_off_ : amb_off_)[r->second];
  const int rows = sz[ia], cols = sz[ib];
  if (ia <= ib) { std::memcpy(out, src, (size_t)rows * cols * sizeof(double)); return SK_OK; }
  for (int i = 0; i < rows; ++i) for (int j = 0; j < cols; ++j) out[(size_t)i * cols + j] = src[(size_t)j * rows + i];  // stored as (ib, ia)
  return SK_OK;
}

int Covariance::get_matrix(double* const* blocks, int n, bool tangent, double* out) const {
  if (!valid_) { set_error("Covariance: no covariance has been computed (call compute first; a failed compute leaves none)"); return SK_ERR_INVALID_ARGUMENT; }
  if (n <= 0 || !blocks || !out) { set_error("Covariance: bad arguments"); return SK_ERR_INVALID_ARGUMENT; }
  const std::vector<int>& sz = tangent ? tangent_ : size_;
  std::vector<int> idx(n), off(n + 1, 0);
  for (int i = 0; i < n; ++i) {
    auto it = block_of_.find(blocks[i]);
    if (it == block_of_.end()) { set_error("Covariance: blocks[%d] is no parameter block of the problem the covariance was computed for", i); return SK_ERR_INVALID_ARGUMENT; }
    idx[i] = it->second; off[i + 1] = off[i] + sz[idx[i]];
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j)
      if (!req_of_.count({std::min(idx[i], idx[j]), std::max(idx[i], idx[j])})) {
        set_error("Covariance: the covariance of blocks[%d] and blocks[%d] was not computed", i, j);
        return SK_ERR_INVALID_ARGUMENT;
      }
  const size_t dim = (size_t)off[n];
  double tile[kCovarianceTile];
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      const int rc = get_block(blocks[i], blocks[j], tangent, tile);
      if (rc != SK_OK) return rc;
      const int rows = sz[idx[i]], cols = sz[idx[j]];
      for (int a = 0; a < rows; ++a) std::memcpy(out + (size_t)(off[i] + a) * dim + off[j], tile + (size_t)a * cols, (size_t)cols * sizeof(double));
    }
  return SK_OK;
}

int Covariance::block_sizes(const double* block, int* size, int* tangent_size) const {
  if (!valid_) { set_error("Covariance: no covariance has been computed (call compute first; a failed compute leaves none)"); return SK_ERR_INVALID_ARGUMENT; }
  auto it = block_of_.find(block);
  if (it == block_of_.end()) { set_error("Covariance: not a parameter block of the problem the covariance was computed for"); return SK_ERR_INVALID_ARGUMENT; }
  if (size) *size = size_[it->second];
  if (tangent_size) *tangent_size = tangent_[it->second];
  return SK_OK;
}

int Covariance::stat(const char* name, double* value) const {
  if (!name || !value) { set_error("null argument"); return SK_ERR_INVALID_ARGUMENT; }
  auto it = stats_.find(name);
  if (!has_stats_ || it == stats_.end()) { set_error("Covariance: no stat \"%s\" (%s)", name, has_stats_ ? "unknown name" : "nothing has been computed"); return SK_ERR_INVALID_ARGUMENT; }
  *value = it->second;
  return SK_OK;
}

int covariance_border_route(int n, const double* H, int block, const int* sel_blocks, int num_sel, double* out, double* ratio_out) {
  if (n <= 0 || !H || block <= 0 || block > kCovarianceMaxBlock || !sel_blocks || num_sel <= 0 || !out) { set_error("invalid argument"); return SK_ERR_INVALID_ARGUMENT; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available: libskeres_amd has no CPU fallback"); return SK_ERR_NO_DEVICE; }
  const int nblocks = (n + block - 1) / block;
  std::vector<ParamBlock> pblocks(nblocks);
  for (int b = 0; b < nblocks; ++b) {
    ParamBlock& pb = pblocks[b];
    pb.type = kParamIdentity; pb.global_size = pb.local_size = std::min(block, n - b * block);
    pb.constant_mask = 0u; pb.global_off = pb.local_off = b * block;
  }
  std::vector<int> sel_col, sel_off(1, 0), ra, rb, a, b;
  std::vector<long> tan_off, amb_off;
  for (int i = 0; i < num_sel; ++i) {
    if (sel_blocks[i] < 0 || sel_blocks[i] >= nblocks) { set_error("invalid argument"); return SK_ERR_INVALID_ARGUMENT; }
    for (int j = 0; j < i; ++j) if (sel_blocks[j] == sel_blocks[i]) { set_error("invalid argument"); return SK_ERR_INVALID_ARGUMENT; }
    for (int j = 0; j < pblocks[sel_blocks[i]].local_size; ++j) sel_col.push_back(sel_blocks[i] * block + j);
    sel_off.push_back((int)sel_col.size());
  }
  const int k = (int)sel_col.size();
  long out_size = 0;
  for (int i = 0; i < num_sel; ++i)
    for (int j = 0; j <= i; ++j) {  // the lower block triangle, mirrored below
      ra.push_back(sel_off[i]); rb.push_back(sel_off[j]); a.push_back(sel_blocks[i]); b.push_back(sel_blocks[j]);
      const long sz = (long)pblocks[sel_blocks[i]].local_size * pblocks[sel_blocks[j]].local_size;
      tan_off.push_back(out_size); out_size += sz;
      amb_off.push_back(out_size); out_size += sz;
    }
  StreamGuard sg;
  SK_HIP_TRY(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
  hipStream_t s = sg.s;
  Bordered B;
  int rc = B.alloc(n, sel_col, s);
  if (rc != SK_OK) return rc;
  std::vector<double> lower((size_t)n * n, 0.0);  // (what the assembly leaves: the lower triangle, zeros above it)
  for (int i = 0; i < n; ++i) std::memcpy(&lower[(size_t)i * n], H + (size_t)i * n, (size_t)(i + 1) * sizeof(double));
  SK_HIP_TRY(hipMemcpy2DAsync(B.S.p, (size_t)B.ld * sizeof(double), lower.data(), (size_t)n * sizeof(double), (size_t)n * sizeof(double), (size_t)n, hipMemcpyHostToDevice, s));
  DevBuf<int> d_ra, d_rb, d_a, d_b; DevBuf<long> d_tan_off, d_amb_off; DevBuf<double> d_x, d_out; DevBuf<ParamBlock> d_pblocks;
  const std::vector<double> x((size_t)n, 0.0);
  SK_HIP_TRY(d_ra.upload(ra, s)); SK_HIP_TRY(d_rb.upload(rb, s)); SK_HIP_TRY(d_a.upload(a, s)); SK_HIP_TRY(d_b.upload(b, s));
  SK_HIP_TRY(d_tan_off.upload(tan_off, s)); SK_HIP_TRY(d_amb_off.upload(amb_off, s)); SK_HIP_TRY(d_x.upload(x, s)); SK_HIP_TRY(d_pblocks.upload(pblocks, s));
  SK_HIP_TRY(d_out.alloc((size_t)out_size)); SK_HIP_TRY(d_out.zero(s));
  int zero = INT_MAX;
  rc = B.scale_and_factor(s, &zero, nullptr);
  if (rc != SK_OK) return rc;
  if (zero != INT_MAX) { set_error("a diagonal entry is zero (column %d)", zero); return SK_ERR_EVALUATION_FAILED; }
  CovRequests R;
  R.num = (int)ra.size(); R.ra = d_ra.p; R.rb = d_rb.p; R.a = d_a.p; R.b = d_b.p; R.tan_off = d_tan_off.p; R.amb_off = d_amb_off.p; R.pblocks = d_pblocks.p; R.x = d_x.p;
  launch_cov_extract(R, B.border(), B.ld, B.d.p, d_out.p, s);
  SK_HIP_TRY(hipGetLastError());
  std::vector<double> packed((size_t)out_size);
  double ratio[2] = {0, 0};
  int info = 0;
  SK_HIP_TRY(hipMemcpyAsync(packed.data(), d_out.p, packed.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  SK_HIP_TRY(hipMemcpyAsync(ratio, B.ratio.p, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
  SK_HIP_TRY(hipMemcpyAsync(&info, B.info.p, sizeof(int), hipMemcpyDeviceToHost, s));
  SK_HIP_TRY(hipStreamSynchronize(s));
  if (info != 0) { set_error("matrix is not positive definite"); return SK_ERR_EVALUATION_FAILED; }
  if (ratio_out) *ratio_out = ratio[1] > 0.0 ? ratio[0] / ratio[1] : 0.0;
  size_t r = 0;
  for (int i = 0; i < num_sel; ++i)
    for (int j = 0; j <= i; ++j, ++r) {
      const int rows = pblocks[sel_blocks[i]].local_size, cols = pblocks[sel_blocks[j]].local_size;
      const double* t = packed.data() + amb_off[r];  // (identity blocks: the lift is a copy — the route is checked through it)
      for (int p = 0; p < rows; ++p)
        for (int q = 0; q < cols; ++q) {
          out[(size_t)(sel_off[i] + p) * k + sel_off[j] + q] = t[(size_t)p * cols + q];
          out[(size_t)(sel_off[j] + q) * k + sel_off[i] + p] = t[(size_t)p * cols + q];
        }
    }
  return SK_OK;
}

}  // namespace sk

#ifdef SK_TESTING
// the testing library's entry to steps 3 to 6 (libskeres_amd_testing.so only; not part of include/skeres_amd.h)
extern "C" int sk_testing_covariance_border_route(int n, const double* H, int block, const int* sel_blocks, int num_sel, double* out, double* ratio) {
  try { return sk::covariance_border_route(n, H, block, sel_blocks, num_sel, out, ratio); }
  catch (...) { sk::set_error("internal error"); return SK_ERR_INVALID_ARGUMENT; }
}
#endif
