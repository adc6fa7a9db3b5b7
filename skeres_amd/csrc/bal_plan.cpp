// Host planning of the DENSE_SCHUR path (bal_plan.hpp): from host data alone, no device.
#include "bal_plan.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <limits>
#include <map>
#include <numeric>
#include <thread>

namespace sk {

// The block structure DENSE_SCHUR eliminates: every residual block has r residuals over TWO parameter blocks, a "camera" of c
// coordinates (the f-block that stays in the reduced system) and a "point" of q coordinates (the e-block that is eliminated),
// the same (r; c, q) for every block, with r <= 2, c <= 9, q <= 3.  The kernels are written for the reference's bundle
// adjuster, (2; 9, 3) (EX/SimpleBundleAdjuster.scala:79-119); a smaller shape — a pinhole camera of six coordinates, a planar
// point — runs in the same kernels PADDED: the missing coordinates are inert unknowns (Jacobi scale 0, as a coordinate held
// constant by a SubsetParameterization: a zero Jacobian column, min_lm_diagonal / radius on the diagonal, step exactly 0), a
// missing residual row is zero.  The LM trajectory is that of the unpadded problem; the reduced system is 9 C wide instead of c C.
bool bal_block_shape(const Problem& p, int* r, int* c, int* q) {
  if (p.rb_functor.empty()) return false;
  const size_t b0 = 0;
  if (p.rb_pidx_off[b0 + 1] - p.rb_pidx_off[b0] != 2) return false;
  *r = p.rb_num_residuals[b0];
  *c = p.block_size[p.rb_pidx[p.rb_pidx_off[b0]]];
  *q = p.block_size[p.rb_pidx[p.rb_pidx_off[b0] + 1]];
  return true;
}
bool problem_is_bal_shaped(const Problem& p, std::string* why) {
  const size_t nb = p.rb_functor.size();
  if (nb == 0) { *why = "problem has no residual blocks"; return false; }
  int R = 0, Cs = 0, Qs = 0;
  const char* shape_msg = "DENSE_SCHUR is implemented for residual blocks with at most 2 residuals over a camera block of at most 9 and a point block of at most 3 "
                          "parameters, the same sizes for every block (SnavelyReprojectionError on the device, a recorded functor, or any host-callback cost "
                          "function of such a shape); not supported: another shape";
  if (!bal_block_shape(p, &R, &Cs, &Qs) || R < 1 || R > 2 || Cs < 1 || Cs > 9 || Qs < 1 || Qs > 3) { *why = shape_msg; return false; }
  // the registered device functor (2; 9, 3), a recorded functor, or ANY cost function of the shape through the director path
  // (sk_cost_function_new_callback: the caller's Evaluate, run on the host — CORE/CostFunctor.scala:40-51, ceres.i:48)
  for (size_t b = 0; b < nb; ++b) {
    if (p.rb_pidx_off[b + 1] - p.rb_pidx_off[b] != 2 || p.rb_num_residuals[b] != R || p.block_size[p.rb_pidx[p.rb_pidx_off[b]]] != Cs ||
        p.block_size[p.rb_pidx[p.rb_pidx_off[b] + 1]] != Qs) { *why = shape_msg; return false; }
    const CostFunction* cf = b < p.rb_cost.size() ? p.rb_cost[b] : nullptr;
    const bool host_ok = p.rb_functor[b] == SK_FUNCTOR_HOST_CALLBACK && cf && cf->callback;
    const bool tape_ok = p.tape_of_block(b) != nullptr;
    const bool snavely_ok = p.rb_functor[b] == SK_FUNCTOR_SNAVELY_REPROJECTION && R == 2 && Cs == 9 && Qs == 3;
    if (!snavely_ok && !host_ok && !tape_ok) { *why = shape_msg; return false; }
  }
  // one device functor per problem: the evaluation kernels are launched over all device-evaluated observations at once
  int device_functor = -1;
  for (size_t b = 0; b < nb; ++b) {
    if (p.rb_functor[b] == SK_FUNCTOR_HOST_CALLBACK) continue;
    if (device_functor < 0) device_functor = p.rb_functor[b];
    else if (device_functor != p.rb_functor[b]) { *why = "DENSE_SCHUR takes one device functor for all residual blocks (host-callback cost functions may be mixed in): not supported"; return false; }
  }
  if (device_functor >= kTapeFunctorBase && bal_tape_width(*p.tapes[device_functor - kTapeFunctorBase]) == 0) {
    *why = "the recorded functor needs more registers (or captures more doubles) than the device interpreter holds: not supported";
    return false;
  }
  // the Schur path carries identity and subset parameterizations and constant blocks; a quaternion or homogeneous-vector block
  // (a 4-block cannot be a camera or a point here anyway) sends the problem to the alternate solver like any other shape
  for (size_t b = 0; b < p.block_param.size(); ++b)
    if (p.block_param[b] >= 0) {
      const int t = p.params[p.block_param[b]].type;
      if (t != kParamIdentity && t != kParamSubset) {
        *why = "DENSE_SCHUR takes identity and subset parameterizations and constant parameter blocks (quaternion / homogeneous-vector blocks are implemented for DENSE_QR / DENSE_NORMAL_CHOLESKY; not supported here)";
        return false;
      }
    }
  std::vector<char> role(p.block_size.size(), 0);
  for (size_t b = 0; b < nb; ++b) {
    const int c = p.rb_pidx[p.rb_pidx_off[b]], q = p.rb_pidx[p.rb_pidx_off[b] + 1];
    if ((role[c] | 1) != 1 || (role[q] | 2) != 2) { *why = "a parameter block is used both as camera and as point"; return false; }
    role[c] = 1; role[q] = 2;
  }
  return true;
}

// Cameras (parameter slot 0) and points (slot 1) in first-appearance order, the
// per-observation indices, and the partition of points over `world` ranks:
// contiguous runs with (nearly) equal sum of k_p^2, because the Schur work of a
// point is quadratic in its track length k_p.
void bal_index_problem(const Problem& p, std::vector<int>* cam_block, std::vector<int>* pt_block, std::vector<int>* ocam,
                       std::vector<int>* opt) {
  const int Nall = (int)p.rb_functor.size();
  std::vector<int> cam_of_block(p.block_size.size(), -1), pt_of_block(p.block_size.size(), -1);
  ocam->resize(Nall); opt->resize(Nall);
  for (int b = 0; b < Nall; ++b) {
    const int cb = p.rb_pidx[p.rb_pidx_off[b]], pb = p.rb_pidx[p.rb_pidx_off[b] + 1];
    if (cam_of_block[cb] < 0) { cam_of_block[cb] = (int)cam_block->size(); cam_block->push_back(cb); }
    if (pt_of_block[pb] < 0) { pt_of_block[pb] = (int)pt_block->size(); pt_block->push_back(pb); }
    (*ocam)[b] = cam_of_block[cb]; (*opt)[b] = pt_of_block[pb];
  }
}

void bal_partition_points(const std::vector<int>& opt, int num_points, int world, std::vector<int>* cut) {
  std::vector<int> kp(num_points, 0);
  for (int q : opt) kp[q]++;
  cut->assign(world + 1, num_points);
  (*cut)[0] = 0;
  double total = 0.0;
  for (int q = 0; q < num_points; ++q) total += (double)kp[q] * kp[q];
  double acc = 0.0;
  int r = 1;
  for (int q = 0; q < num_points && r < world; ++q) {
    acc += (double)kp[q] * kp[q];
    while (r < world && acc >= total * r / world) (*cut)[r++] = q + 1;
  }
}

// ---- camera ordering for the reduced system --------------------------------------------------------------
// The order of the cameras inside S is the solver's to choose (Ceres, too, orders the blocks of the reduced
// system itself).  A block-banded S factors in a fraction of the flops of a full one (cholesky_factor's
// envelope), and whether S is banded depends on that order alone.  Candidates: first appearance in the residual
// blocks (what bal_index_problem yields), memory order of the camera blocks (the BAL file's numbering when the
// caller uses the reference's layout, EX/SimpleBundleAdjuster.scala:18-34), and reverse Cuthill-McKee on the
// co-visibility graph.  The one with the fewest trailing-update flops wins; ties keep the earlier candidate.
static std::vector<int> envelope_of_order(const std::vector<int>& ocam, const std::vector<int>& opt, const std::vector<int>& new_id, int C, int P,
                                          int nblk, std::vector<int>* first_col_out = nullptr) {
  std::vector<int> cmin(P, C);
  for (size_t b = 0; b < ocam.size(); ++b) cmin[opt[b]] = std::min(cmin[opt[b]], new_id[ocam[b]]);
  std::vector<int> first_col(nblk);
  for (int i = 0; i < nblk; ++i) first_col[i] = i;
  for (size_t b = 0; b < ocam.size(); ++b) {  // camera c shares point opt[b] with camera cmin: block (rows of c, columns of cmin)
    const int c = new_id[ocam[b]], col = (9 * cmin[opt[b]]) / 128;
    for (int row = (9 * c) / 128; row <= (9 * c + 8) / 128; ++row) first_col[row] = std::min(first_col[row], col);
  }
  if (first_col_out) *first_col_out = first_col;
  return cholesky_envelope_last(first_col);
}

// ---- two-way dissection of the camera sequence (the dissected factorisation of the Cholesky kernels, "Two-way dissection") ---------------------------------
// Cameras in the chosen (banded) order: head [0, a), separator [a, b), tail [b, C), with no point seen from both the head
// and the tail: b = 1 + the last camera that shares a point with a camera before a.  The head is eliminated front to back
// and the tail back to front, side by side, so the serial panel chain is about half as long.  Where to cut is decided
// by a model of the two chains (microseconds per block column; constants measured on MI355X, profiles/r02_*): a block
// column costs the larger of its panel chain and its trailing update.
struct Dissection { int a = 0, b = 0; double t_plain = 0.0, t_dissected = 0.0; };
// ---- the chain model: microseconds per block column of a factorisation, constants measured on MI355X ----------------------
// Round 5: recalibrated on the bench line's chain_model records of round 4 (measured / model was 1.22-1.47 on the plans with retained
// points — every column chain-bound, two fronts in lock-step — 0.98 with every point eliminated, 0.83-0.89 on wide envelopes).
// A chain-bound column's cycle is the LONGER of the panel chain and the thin trailing SYRK it overlaps with, which the next column
// launch but one waits for (180 tiles 21 us, 760 tiles 49 us: profiles/r04_factor_timeline*.txt; "40-50 us up to 13 trailing rows, 60
// at 20, 100 at 30" of round 1 is the same line); wide updates run at 38 TFLOP/s at a few dozen block rows and at 44-46 towards a full
// matrix (roofline_full: 44.9); the back-substitution is part of the phase the model is held against.
namespace chain_model {
constexpr int kChainBoundRows = 24;          // block rows below the diagonal up to which a block column is chain-bound; also the widest separator (in blocks) that is one
constexpr double kChainUs = 40.0;            // the panel chain of one resident block column
constexpr double kPairChainUs = 44.5;        // ... when two fronts share the launches (the lock-step dissection)
constexpr double kThinSyrkUs = 12.0, kThinSyrkUsPerTile = 0.049;  // the thin trailing SYRK: a launch + per 32 x 128 tile
constexpr double kHandOverUs = 8.0;          // ... and its hand-over to the next column launch
constexpr double kLaunchedColumnUs = 70.0, kLaunchedFlopsPerUs = 14e6;  // a chain-bound column factored launch by launch (four launches per column)
constexpr double kWideTflopsMin = 34.0, kWideTflopsPerRow = 0.12, kWideTflopsMax = 46.0, kWideColumnUs = 14.0;  // a SYRK-bound column
constexpr double kBacksolveUs = 20.0, kBacksolveUsPerColumn = 3.3;  // a resident back-substitution launch, per block column
constexpr double kAllreduceUs = 50.0;        // the latency of the reduced system's all-reduce (a small, latency-bound one: 40)
constexpr double kSmallAllreduceUs = 40.0;
constexpr double kLinkBytesPerUs = 153e3;    // a ring over one xGMI link per direction
constexpr double kBlockBytes = 128.0 * 128.0 * 8.0;
bool chain_bound(int h) { return h <= kChainBoundRows; }
double thin_syrk_us(double tiles) { return tiles > 0.0 ? kThinSyrkUs + kThinSyrkUsPerTile * tiles : 0.0; }
double thin_tiles(int h) { return h > 1 ? 2.0 * (h - 1.0) * h : 0.0; }  // 32 x 128 tiles of the trailing update behind the next block column: h - 1 block rows, lower triangle
double column_cost_us(int h, bool resident_capable) {
  const double flops = 128.0 * 128.0 * 128.0 * ((double)h * h + h);
  if (resident_capable && chain_bound(h)) return std::max(kChainUs, thin_syrk_us(thin_tiles(h)) + kHandOverUs);
  if (chain_bound(h)) return std::max(kLaunchedColumnUs, flops / kLaunchedFlopsPerUs);
  return flops / (std::min(kWideTflopsMax, kWideTflopsMin + kWideTflopsPerRow * h) * 1e6) + kWideColumnUs;
}
// two chain-bound block columns, one of each leaf front, in ONE column launch and ONE thin SYRK (the lock-step dissection)
double pair_cost_us(int h1, int h2) { return std::max(kPairChainUs, thin_syrk_us(thin_tiles(h1) + thin_tiles(h2)) + kHandOverUs); }
double backsolve_us(int block_columns) { return block_columns > 0 ? kBacksolveUs + kBacksolveUsPerColumn * block_columns : 0.0; }
// The bandwidth term of an all-reduce over `world` ranks (2 (W - 1) / W x the bytes over the link) of `blocks` 128-blocks, and of the
// lower triangle of block_rows block rows — 39 MB and 0.4 ms for ONE 24-block separator, which is what keeps a second wide separator
// from paying on the Ladybug-shaped problem.  (Two functions: the products are formed in the order the plans were calibrated with.)
double allreduce_blocks_us(double blocks, int world) { const int W = std::max(2, world); return 2.0 * (W - 1.0) / W * blocks * kBlockBytes / kLinkBytesPerUs; }
double allreduce_triangle_us(double block_rows, int world) {
  const int W = std::max(2, world);
  return 2.0 * (W - 1.0) / W * 0.5 * block_rows * (block_rows + 1.0) * kBlockBytes / kLinkBytesPerUs;
}
// Seconds on one MI355X of the phases that shard with the points (Jacobians, Schur assembly, back-substitution, candidate cost).  Round 5:
// recalibrated on the bench records — Ladybug-1723 0.66 ms (679 k observations, 2.4 M pair entries), Venice-1778 3.65 ms (5.0 M, 25 M);
// round 1's constants (0.15 ns per pair entry + 1.9 ns per observation) were those kernels three rounds ago
double shardable_work_s(double pairs, double observations) { return 0.03e-9 * pairs + 0.6e-9 * observations; }
double pair_entries(const std::vector<int>& opt, int num_points) {
  std::vector<int> k(num_points, 0);
  for (int v : opt) k[v]++;
  double pairs = 0.0;
  for (int v : k) pairs += 0.5 * (double)v * (double)(v - 1);
  return pairs;
}
}  // namespace chain_model
using namespace chain_model;
// tail_resident: the tail has a device of its own (segmented world) and runs under a resident panel chain like the head;
// on one device it is factored launch by launch next to the head's chain.
// lockstep: the schedule of ONE device since the end of round 3 — the tail's block columns ride in the launches of the head's
// trailing run of chain-bound columns (CholeskyPartner), so a paired step costs the dearer of its two columns and the head's
// block columns before that run are not shortened at all.
// extra_sep: cameras that join the separator whatever the cut (the pseudo-cameras of retained points, which every camera may couple with)
// extra_fwd (optional, per block column of the band): border block rows that are active in that column on top of its run — the tail
// profile of the bordered envelope — when the head is eliminated front to back; extra_bwd: the same for the tail front, for which the
// profile is not known (its columns reach the border's rows in another order): all of them.
// reach[c]: the last camera that shares a point with any camera <= c (cameras in the chosen order) — what a cut behind camera c - 1 needs
// as its separator's end.  Three passes over the observations: a caller that plans several cuts of one sequence forms it once (reach_in).
static std::vector<int> camera_reach(const std::vector<int>& ocam, const std::vector<int>& opt, int C, int P) {
  std::vector<int> cmin(P, C), cmax(P, -1), reach(C);
  for (size_t b = 0; b < ocam.size(); ++b) { cmin[opt[b]] = std::min(cmin[opt[b]], ocam[b]); cmax[opt[b]] = std::max(cmax[opt[b]], ocam[b]); }
  for (int c = 0; c < C; ++c) reach[c] = c;
  for (int q = 0; q < P; ++q) if (cmax[q] >= 0) reach[cmin[q]] = std::max(reach[cmin[q]], cmax[q]);
  for (int c = 1; c < C; ++c) reach[c] = std::max(reach[c], reach[c - 1]);
  return reach;
}
static Dissection choose_dissection(const std::vector<int>& ocam, const std::vector<int>& opt, int C, int P, int nblk, const std::vector<int>& last,
                                    const std::vector<int>& first_col, bool tail_resident, bool lockstep = false, int extra_sep = 0,
                                    const std::vector<int>* extra_fwd = nullptr, int extra_bwd = 0, const std::vector<int>* extra_bwd_col = nullptr,
                                    const std::vector<int>* reach_in = nullptr) {
  Dissection d;
  if (C < 64 || nblk < 24) return d;
  // reach[c]: the last camera that shares a point with any camera <= c (cameras in the chosen order)
  const std::vector<int> reach_own = reach_in ? std::vector<int>() : camera_reach(ocam, opt, C, P);
  const std::vector<int>& reach = reach_in ? *reach_in : reach_own;
  // per block column: height forward (rows below, as the envelope has it) and backward (rows above: the tail's view)
  std::vector<double> fwd(nblk), bwd(nblk), fwd_sum(nblk + 1, 0.0), bwd_sum(nblk + 1, 0.0);
  std::vector<int> height(nblk), height_b(nblk);
  std::vector<int> fc(first_col);
  for (int i = nblk - 2; i >= 0; --i) fc[i] = std::min(fc[i], fc[i + 1] < i + 1 ? fc[i + 1] : i);  // (monotone, as the backward envelope is)
  for (int c = 0; c < nblk; ++c) {
    const int hf = std::min(last[c], nblk - 1) - c + (last[c] < nblk - 1 ? 1 : 0) + (extra_fwd && c < (int)extra_fwd->size() ? (*extra_fwd)[c] : 0);
    height[c] = hf;
    fwd[c] = column_cost_us(hf, true);
    height_b[c] = c - std::min(fc[c], c) + 1 + (extra_bwd_col && c < (int)extra_bwd_col->size() ? (*extra_bwd_col)[c] : extra_bwd);
    bwd[c] = column_cost_us(height_b[c], tail_resident);
    d.t_plain += fwd[c];
  }
  d.t_plain += backsolve_us(nblk + (extra_sep > 0 ? (9 * extra_sep + 127) / 128 : 0));
  for (int c = 0; c < nblk; ++c) { fwd_sum[c + 1] = fwd_sum[c] + fwd[c]; bwd_sum[c + 1] = bwd_sum[c] + bwd[c]; }
  double best = d.t_plain;
  for (int a = 14; a + 14 < C; a += 7) {
    const int b = reach[a - 1] + 1;
    if (b >= C - 14) break;
    const int ca = (9 * a + 127) / 128, cb = (9 * b) / 128, E = (9 * (b - a + extra_sep) + 1 + 127) / 128;
    if (E > kChainBoundRows) continue;  // a separator that wide is no separator: its dense system is factored after both chains, alone
    double root = 0.0;
    for (int i = 0; i < E; ++i) root += column_cost_us(E - 1 - i, true);
    // (+ the back-substitutions: the root's, then the two interiors side by side)
    const double bs = backsolve_us(E) + backsolve_us(std::max(ca, nblk - cb)) + 20.0;
    double t = std::max(fwd_sum[ca], bwd_sum[nblk] - bwd_sum[cb]) + root + 120.0 + bs;  // + fork, join, border add
    if (lockstep) {
      // the head's chain-bound columns (its first few, and its trailing run) each carry one of the tail's; the others cost what they cost
      const int nb = nblk - cb;
      int k = 0;
      t = root + 100.0 + bs;  // + border add, the root's own start and join (180 us until the chain's starts and joins lost their events: round 5)
      for (int c = 0; c < ca; ++c) {
        if (chain_bound(height[c]) && k < nb) { t += chain_bound(height_b[nblk - 1 - k]) ? pair_cost_us(height[c], height_b[nblk - 1 - k]) : std::max(fwd[c], bwd[nblk - 1 - k]); ++k; }
        else t += fwd[c];
      }
      for (; k < nb; ++k) t += bwd[nblk - 1 - k];
    }
    if (t < best) { best = t; d.a = a; d.b = b; }
  }
  d.t_dissected = best;
  // (the lock-step schedule adds no queues and no second chain's interference: it is taken for half the predicted gain the
  // side-by-side one needed — measured on Ladybug-1723: predicted 9.8 %, 2.3 % of the iteration in the bench line)
  if (best > (lockstep ? 0.95 : 0.9) * d.t_plain) { d.a = d.b = 0; }
  return d;
}

// Block envelope of one front: `pos[c]` is camera c's first row in the front (interior or border), -1 when the camera has
// no rows in it; `interior[c]` whether its columns are eliminated in this front.  Only points that touch an interior
// camera shape the envelope (the border x border block is the Schur complement's, covered by the last columns' reach).
// tail_begin_row >= 0: the front's rows from there on (the rows of retained points, at the end of its border) are a border in the sense
// of cholesky_envelope_bordered — active from the first column that reaches them, not part of a column's contiguous run: *tail_out.
static std::vector<int> front_envelope(const std::vector<int>& ocam, const std::vector<int>& opt, const std::vector<int>& pos, const std::vector<char>& interior,
                                       int P, int nblk, int tail_rows = 1, int tail_begin_row = -1, std::vector<int>* tail_out = nullptr) {
  const int kNone = 1 << 30;
  std::vector<int> minpos(P, kNone);
  for (size_t b = 0; b < ocam.size(); ++b) if (interior[ocam[b]]) minpos[opt[b]] = std::min(minpos[opt[b]], pos[ocam[b]]);
  std::vector<int> first_col(nblk);
  for (int i = 0; i < nblk; ++i) first_col[i] = i;
  for (size_t b = 0; b < ocam.size(); ++b) {
    const int c = ocam[b];
    if (pos[c] < 0 || minpos[opt[b]] == kNone) continue;
    const int col = minpos[opt[b]] / 128;
    for (int row = pos[c] / 128; row <= (pos[c] + 8) / 128; ++row) first_col[row] = std::min(first_col[row], std::min(col, row));
  }
  if (tail_begin_row >= 0 && tail_out) {
    std::vector<int> last;
    cholesky_envelope_bordered(first_col, tail_begin_row / 128, &last, tail_out);
    return last;
  }
  return cholesky_envelope_last(first_col, tail_rows);
}

// ---- multi-way dissection over the ranks of a world ---------------------------------------------------
// R segments of the camera sequence with a separator between neighbours: separator k (1 <= k < R) = cameras [a[k-1], b[k-1])
// of the banded numbering, b = 1 + the last camera that shares a point with a camera before a.  Every segment is
// eliminated on a device of its own — the last one back to front, the others front to back — and the separators'
// block-tridiagonal system by every rank.  The cuts balance the segments' chains under the same model of a block
// column's cost as choose_dissection; the number of segments (at most max_segments) is the one with the shortest
// predicted critical path.  forced: cut wherever separators exist (tests, small problems), as evenly as the sequence allows.
struct Segments { std::vector<int> a, b; double t_plain = 0.0, t_model = 0.0; double model_us[9] = {0}; };
// member_cams: cameras that join the root whatever the cuts (the border's members: pseudo-cameras of retained points, loop-closure cameras) —
// rows of EVERY segment's front, active in a block column as extra_fwd / extra_bwd_col have it (as in choose_dissection), and a border of the root.
static Segments choose_segments(const std::vector<int>& ocam, const std::vector<int>& opt, int C, int P, int nblk, const std::vector<int>& last,
                                const std::vector<int>& first_col, int max_segments, bool forced, int world = 0, int member_cams = 0,
                                const std::vector<int>* extra_fwd = nullptr, const std::vector<int>* extra_bwd_col = nullptr,
                                const std::vector<int>* reach_in = nullptr) {
  Segments out;
  const int mb = member_cams > 0 ? (9 * member_cams + 127) / 128 : 0;
  if (world <= 0) world = max_segments;
  max_segments = std::min(max_segments, 8);
  if (max_segments < 2 || C < 6) return out;
  const std::vector<int> reach_own = reach_in ? std::vector<int>() : camera_reach(ocam, opt, C, P);
  const std::vector<int>& reach = reach_in ? *reach_in : reach_own;
  if (C >= 64 && nblk >= 24) {
    std::vector<double> fwd(nblk), bwd(nblk), fwd_sum(nblk + 1, 0.0), bwd_sum(nblk + 1, 0.0);
    std::vector<int> fc(first_col);
    for (int i = nblk - 2; i >= 0; --i) fc[i] = std::min(fc[i], fc[i + 1] < i + 1 ? fc[i + 1] : i);
    for (int c = 0; c < nblk; ++c) {
      const int hf = std::min(last[c], nblk - 1) - c + (last[c] < nblk - 1 ? 1 : 0) + (extra_fwd && c < (int)extra_fwd->size() ? (*extra_fwd)[c] : mb);
      fwd[c] = column_cost_us(hf, true);
      bwd[c] = column_cost_us(c - std::min(fc[c], c) + 1 + (extra_bwd_col && c < (int)extra_bwd_col->size() ? (*extra_bwd_col)[c] : mb), true);
      out.t_plain += fwd[c];
    }
    for (int i = 0; i < mb; ++i) out.t_plain += column_cost_us(mb - 1 - i, true);
    for (int c = 0; c < nblk; ++c) { fwd_sum[c + 1] = fwd_sum[c] + fwd[c]; bwd_sum[c + 1] = bwd_sum[c] + bwd[c]; }
    out.model_us[1] = out.t_plain + backsolve_us(nblk + mb);
    const double plain_with_solve = out.model_us[1];
    auto sep_blocks = [&](int a) { return (9 * (reach[a - 1] + 1 - a) + 1 + 127) / 128; };
    // room[k]: the last camera at which a segment may START so that k more cuts (each a candidate below, each followed by a
    // segment of at least 14 cameras) still fit behind it
    std::vector<int> room(9, -1);
    room[0] = C - 15;
    for (int k = 1; k <= 8; ++k)
      for (int a = 14; a + 14 < C; a += 7) {
        const int b = reach[a - 1] + 1;
        if (b >= C - 14) break;
        if (sep_blocks(a) <= kChainBoundRows && b <= room[k - 1]) room[k] = std::max(room[k], a - 14);
      }
    // can the sequence be cut into Rn segments none of whose chains is longer than T?  Greedy: every segment as long as T allows.
    auto plan_for = [&](int Rn, double T, std::vector<int>* as) {
      int pos = 0;
      as->clear();
      for (int sgm = 0; sgm + 1 < Rn; ++sgm) {
        int best_a = -1;
        for (int a = ((pos + 14 + 6) / 7) * 7; a + 14 < C; a += 7) {
          const int b = reach[a - 1] + 1;
          if (b >= C - 14) break;
          if (b > room[Rn - 2 - sgm]) continue;  // (room for the cuts still to come: a generous T must not spend the whole sequence on this segment)
          if (fwd_sum[(9 * a + 127) / 128] - fwd_sum[(9 * pos) / 128] > T) break;
          if (sep_blocks(a) <= kChainBoundRows) best_a = a;
        }
        if (best_a < 0) return false;
        as->push_back(best_a);
        pos = reach[best_a - 1] + 1;
      }
      return bwd_sum[nblk] - bwd_sum[(9 * pos) / 128] <= T;
    };
    double best = plain_with_solve;
    std::vector<int> best_as;
    for (int Rn = 2; Rn <= max_segments; ++Rn) {
      std::vector<int> as;
      if (!plan_for(Rn, out.t_plain, &as)) break;
      double lo = 0.0, hi = out.t_plain;
      for (int it = 0; it < 40; ++it) { const double mid = 0.5 * (lo + hi); if (plan_for(Rn, mid, &as)) hi = mid; else lo = mid; }
      (void)plan_for(Rn, hi, &as);
      double root = 0.0;  // the separators' block-tridiagonal system, one resident column after the other, on every rank
      for (size_t k = 0; k < as.size(); ++k) {
        const int E = sep_blocks(as[k]), Enext = k + 1 < as.size() ? sep_blocks(as[k + 1]) : 0;
        for (int i = 0; i < E; ++i) root += column_cost_us(E - 1 - i + Enext + mb, true);
      }
      for (int i = 0; i < mb; ++i) root += column_cost_us(mb - 1 - i, true);  // (the members: a dense border of the root)
      // + the all-reduce of the root over the world's ranks: its lower triangle inside the block-tridiagonal envelope, a ring over
      // one xGMI link per direction (chain_model::allreduce_blocks_us)
      double blocks = 0.0;
      for (size_t k = 0; k < as.size(); ++k) {
        const double E = sep_blocks(as[k]), Eprev = k > 0 ? sep_blocks(as[k - 1]) : 0.0;
        blocks += 0.5 * E * (E + 1.0) + E * Eprev + E * mb;
      }
      blocks += 0.5 * mb * (mb + 1.0);
      const double allreduce_us = kAllreduceUs + allreduce_blocks_us(blocks, world);
      int root_blocks = mb;
      for (size_t k = 0; k < as.size(); ++k) root_blocks += sep_blocks(as[k]);
      const double t = hi + root + 170.0 + allreduce_us + backsolve_us(root_blocks) + backsolve_us((nblk + Rn - 1) / Rn);  // + fork, join, border add; the root's and a segment's back-substitution
      out.model_us[Rn] = t;
      if (dev_knobs().debug_segments) std::fprintf(stderr, "[skeres_amd] %d segments: longest chain %.0f us, root %.0f us, all-reduce %.0f us (%.0f blocks) -> %.0f us (undissected %.0f)\n", Rn, hi, root, allreduce_us, blocks, t, out.t_plain);
      // (forced: a segment per rank, as far as the sequence can be cut; otherwise a further segment has to beat the plan so far by
      // 5 %: the model is no better than that, and every separator is more to all-reduce and to factor on every rank)
      if (forced ? true : t < best * (Rn > 2 ? 0.95 : 1.0)) { best = t; best_as = as; }
    }
    out.t_model = best;
    if (!best_as.empty() && (forced || best <= 0.9 * plain_with_solve)) {
      for (int a : best_as) { out.a.push_back(a); out.b.push_back(reach[a - 1] + 1); }
      return out;
    }
  }
  if (!forced) return out;
  for (int Rn = max_segments; Rn >= 2 && out.a.empty(); --Rn) {
    std::vector<int> as, bs;
    int pos = 0;
    bool ok = true;
    for (int k = 1; k < Rn && ok; ++k) {
      // the cut nearest to the k-th Rn-th of the sequence (from there towards the front) whose separator leaves room behind it
      int a = std::min(C - 1, std::max(pos + 1, (int)((long)k * C / Rn)));
      while (a > pos && reach[a - 1] + 1 >= C - (Rn - 1 - k)) --a;
      if (a <= pos) { ok = false; break; }
      as.push_back(a); bs.push_back(reach[a - 1] + 1);
      pos = bs.back();
    }
    if (ok && pos < C) { out.a = as; out.b = bs; }
  }
  return out;
}

// f(i) for i in [0, n) on up to twelve host threads (the caller's among them).  The planner's candidates — each a handful of passes over every
// observation — are independent of each other; which one is taken is decided afterwards, in the candidates' own order, so the plan does not
// depend on the number of threads (round 5: the plan of the reduced system was 0.7 s of Ladybug-1723's 0.8 s of set-up, 8 s of Venice-1778's 9).
static std::atomic<int> g_plan_helpers{0};  // helper threads of the planner alive in this process (nested calls share one budget)
template <class F>
static void plan_parallel_for(int n, F f) {
  const int budget = std::min(12, std::max(1, (int)std::thread::hardware_concurrency())) - 1;
  int helpers = 0;
  while (helpers < n - 1) {  // (claim helper threads one by one, as far as the budget goes)
    int cur = g_plan_helpers.load();
    if (cur >= budget) break;
    if (g_plan_helpers.compare_exchange_weak(cur, cur + 1)) ++helpers;
  }
  if (helpers == 0) { for (int i = 0; i < n; ++i) f(i); return; }
  std::atomic<int> next{0};
  auto work = [&] { for (int i; (i = next.fetch_add(1)) < n;) f(i); };
  std::vector<std::thread> pool;
  pool.reserve((size_t)helpers);
  for (int t = 0; t < helpers; ++t) {
    try { pool.emplace_back(work); } catch (...) { break; }  // (no thread to be had: the ones there are, and this one, do the work)
  }
  work();
  for (std::thread& t : pool) t.join();
  g_plan_helpers.fetch_sub(helpers);
}
static std::vector<int> rcm_order(const std::vector<int>& ocam, const std::vector<int>& opt, int C, int P) {
  // co-visibility graph, thinned: the cameras of a point are chained in index order and the ends joined
  // (the cameras of every point as flat sorted lists — a counting sort and one small sort per point)
  std::vector<int> pstart((size_t)P + 1, 0), pcam(ocam.size());
  for (int q : opt) pstart[(size_t)q + 1]++;
  for (int q = 0; q < P; ++q) pstart[(size_t)q + 1] += pstart[(size_t)q];
  { std::vector<int> fill(pstart.begin(), pstart.end() - 1); for (size_t b = 0; b < ocam.size(); ++b) pcam[(size_t)fill[(size_t)opt[b]]++] = ocam[b]; }
  for (int q = 0; q < P; ++q) std::sort(pcam.begin() + pstart[(size_t)q], pcam.begin() + pstart[(size_t)q + 1]);
  std::vector<std::vector<int>> adj(C);
  if (C <= 16384) {
    // the edge set as a bit matrix (32 MB at 16384 cameras): no list of a few hundred thousand pairs to sort and to thin out
    const size_t words = ((size_t)C + 63) / 64;
    std::vector<unsigned long long> bits((size_t)C * words, 0ull);
    auto edge = [&](int a, int b) { if (a != b) { bits[(size_t)a * words + (size_t)b / 64] |= 1ull << (b % 64); bits[(size_t)b * words + (size_t)a / 64] |= 1ull << (a % 64); } };
    for (int q = 0; q < P; ++q) {
      const int a = pstart[(size_t)q], e = pstart[(size_t)q + 1];
      for (int k = a; k + 1 < e; ++k) edge(pcam[(size_t)k], pcam[(size_t)k + 1]);
      if (e - a > 2) edge(pcam[(size_t)a], pcam[(size_t)e - 1]);
    }
    for (int u = 0; u < C; ++u)
      for (size_t w = 0; w < words; ++w)
        for (unsigned long long m = bits[(size_t)u * words + w]; m; m &= m - 1) adj[(size_t)u].push_back((int)(w * 64) + __builtin_ctzll(m));
  } else {
    std::vector<std::pair<int, int>> edges;
    for (int q = 0; q < P; ++q) {
      const int a = pstart[(size_t)q], e = pstart[(size_t)q + 1];
      for (int k = a; k + 1 < e; ++k) edges.emplace_back(pcam[(size_t)k], pcam[(size_t)k + 1]);
      if (e - a > 2) edges.emplace_back(pcam[(size_t)a], pcam[(size_t)e - 1]);
    }
    std::sort(edges.begin(), edges.end());
    edges.erase(std::unique(edges.begin(), edges.end()), edges.end());
    for (auto& e : edges) if (e.first != e.second) { adj[e.first].push_back(e.second); adj[e.second].push_back(e.first); }
  }
  for (auto& a : adj) std::sort(a.begin(), a.end(), [&](int x, int y) { return adj[x].size() != adj[y].size() ? adj[x].size() < adj[y].size() : x < y; });
  std::vector<int> order, level(C, -1);
  order.reserve(C);
  auto bfs = [&](int root, std::vector<int>* out) {  // Cuthill-McKee sweep of root's component (unvisited part); returns the last vertex
    const size_t begin = out->size();
    out->push_back(root); level[root] = 0;
    for (size_t h = begin; h < out->size(); ++h) {
      const int u = (*out)[h];
      for (int v : adj[u]) if (level[v] < 0) { level[v] = level[u] + 1; out->push_back(v); }
    }
    return out->back();
  };
  std::vector<char> done(C, 0);
  for (int seed = 0; seed < C; ++seed) {
    if (done[seed]) continue;
    // pseudo-peripheral start: two sweeps, each restarting from the far end of the previous one
    int root = seed;
    for (int rep = 0; rep < 2; ++rep) {
      std::vector<int> tmp;
      const int far = bfs(root, &tmp);
      for (int v : tmp) level[v] = -1;
      root = far;
    }
    const size_t begin = order.size();
    bfs(root, &order);
    for (size_t h = begin; h < order.size(); ++h) done[order[h]] = 1;
  }
  std::reverse(order.begin(), order.end());
  std::vector<int> new_id(C);
  for (int k = 0; k < C; ++k) new_id[order[k]] = k;
  return new_id;
}

// The candidate orders of the cameras inside the reduced system and the one with the fewest trailing-update flops (ties keep
// the earlier candidate).  with_memory_order: host addresses are this process's own — with separately allocated camera
// blocks the order could differ from rank to rank, and the ranks must build the same reduced system: one process only (the
// slot then repeats candidate 0, which keeps the numbering of sk_solver_stat("camera_order")).
static std::vector<std::vector<int>> camera_order_candidates(const Problem& p, const std::vector<int>& cam_block, const std::vector<int>& ocam,
                                                             const std::vector<int>& opt, int C, int P, bool with_memory_order) {
  std::vector<std::vector<int>> cand;
  { std::vector<int> id(C); std::iota(id.begin(), id.end(), 0); cand.push_back(id); }  // first appearance
  if (with_memory_order) {
    std::vector<int> by_addr(C); std::iota(by_addr.begin(), by_addr.end(), 0);
    std::sort(by_addr.begin(), by_addr.end(), [&](int a, int b) { return p.block_ptr[cam_block[a]] < p.block_ptr[cam_block[b]]; });
    std::vector<int> id(C); for (int k = 0; k < C; ++k) id[by_addr[k]] = k; cand.push_back(id);
  } else {
    cand.push_back(cand[0]);
  }
  cand.push_back(rcm_order(ocam, opt, C, P));
  return cand;
}
static void choose_camera_order(const std::vector<std::vector<int>>& cand, const std::vector<int>& ocam, const std::vector<int>& opt, int C, int P, int npad,
                                int* best_k, std::vector<int>* best_env, double* best_flops) {
  double best = -1.0;
  std::vector<std::vector<int>> envs(cand.size());
  std::vector<double> flops(cand.size(), 0.0);
  plan_parallel_for((int)cand.size(), [&](int k) {  // (the candidates' envelopes side by side; the choice in their order)
    envs[(size_t)k] = envelope_of_order(ocam, opt, cand[(size_t)k], C, P, npad / 128);
    flops[(size_t)k] = cholesky_syrk_flops(npad, 1, envs[(size_t)k].data());
  });
  for (size_t k = 0; k < cand.size(); ++k) {
    const double f = flops[k];
    if (best < 0.0 || f < best * (1.0 - 1e-9)) { best = f; *best_k = (int)k; best_env->swap(envs[k]); }
  }
  *best_flops = best;
}

// ---- loop closures: the cameras that revisit a place, ordered into a trailing BORDER (round 4) ------------------------------
// A camera sequence that comes back to a street it has seen couples two distant windows of the band: in the band's own
// order every block column between the two windows is dragged into the envelope (a handful of such tracks fill it: 0.37 ->
// 0.99 of the blocks on the Ladybug-shaped problem).  Numbered BEHIND the band instead, the revisiting cameras are border
// rows — "rows active in every column from the column that first reaches them", the tail profile of cholesky_factor — the
// band keeps its width, and the border's own few block columns are factored last.  Which cameras: in a point's ascending
// camera list a jump of more than `gap` cameras separates visits; the cameras of the later visits (or, the other variant,
// of all visits but the last) go to the border.  Which gap and variant, and whether at all: the chain model of
// choose_dissection (microseconds per block column), over a few gaps; the border is taken when it predicts 10 % less than
// the band's own envelope.  A result of the solve does not depend on the order (EX/SimpleBundleAdjuster.scala:147-152: DENSE_SCHUR
// of Ceres orders its reduced system itself); tests hold the bordered order against the plain one and the oracle.
static double envelope_model_us(int nblk, const std::vector<int>& last, const int* tail) {
  double t = 0.0;
  const BlockEnvelope env(nblk, last.data(), tail);
  for (int c = 0; c < nblk; ++c) t += column_cost_us(env.height(c), true);
  return t + backsolve_us(nblk);
}
// A camera graph: per observation its camera and its point.  Two of them describe a problem with RETAINED points (below): `g`, the
// observations of the points the Schur complement eliminates, over the C real cameras; `x`, the structure of the reduced system —
// g's observations, and for every observation of a retained point a point of its own that couples the observation's camera with
// the retained point's pseudo-camera (index >= g.C).  Without retained points x is g.
static void point_camera_lists(const CamGraph& g, std::vector<int>* pstart, std::vector<int>* pcam) {
  pstart->assign(g.P + 1, 0); pcam->resize(g.ocam->size());
  for (int q : *g.opt) (*pstart)[q + 1]++;
  for (int q = 0; q < g.P; ++q) (*pstart)[q + 1] += (*pstart)[q];
  { std::vector<int> fill(pstart->begin(), pstart->end() - 1); for (size_t b = 0; b < g.ocam->size(); ++b) (*pcam)[fill[(*g.opt)[b]]++] = (*g.ocam)[b]; }
  for (int q = 0; q < g.P; ++q) std::sort(pcam->begin() + (*pstart)[q], pcam->begin() + (*pstart)[q + 1]);
}
// The cameras of every point as lists (point_camera_lists) — what choose_border works on.  A caller that scores many variants of one
// graph (choose_retained_points: the same observations with a few points taken out) forms them once and derives each variant's
// by copying, instead of a counting sort and 150 000 small sorts per variant.
struct PointLists { std::vector<int> start, cam; };
// first_col of envelope_of_order from the lists: block row of every camera of a point <- the block column of the point's first camera
static void first_cols_from_lists(const std::vector<int>& start, const std::vector<int>& cam, const std::vector<int>& new_id, int nblk, std::vector<int>* first_col) {
  first_col->resize((size_t)nblk);
  for (int i = 0; i < nblk; ++i) (*first_col)[(size_t)i] = i;
  const int P = (int)start.size() - 1;
  for (int q = 0; q < P; ++q) {
    const int a = start[(size_t)q], e = start[(size_t)q + 1];
    if (a == e) continue;
    int mn = new_id[(size_t)cam[(size_t)a]];
    for (int k = a + 1; k < e; ++k) mn = std::min(mn, new_id[(size_t)cam[(size_t)k]]);
    const int col = (9 * mn) / 128;
    for (int k = a; k < e; ++k) {
      const int c = new_id[(size_t)cam[(size_t)k]];
      for (int row = (9 * c) / 128; row <= (9 * c + 8) / 128; ++row) (*first_col)[(size_t)row] = std::min((*first_col)[(size_t)row], col);
    }
  }
}
// g, x: cameras in the banded numbering (pseudo-cameras behind the real ones).  mode: SK_BORDER_AUTO (the model decides) / SK_BORDER_ON
// (the best candidate whatever the model says).  gaps_ok: loop-closure cameras may go to the border; pseudo-cameras always do, and with
// them a border is always returned (plain_us is then the model of the border of pseudo-cameras alone).
// gl, xl (optional): the lists of g and of x, formed by the caller — g.ocam / x.ocam may then be null (the lists are all that is read).
static bool choose_border(const CamGraph& g, const CamGraph& x, int nblk, const std::vector<int>& plain_last, int mode, bool gaps_ok, BorderChoice* out,
                          const PointLists* gl = nullptr, const PointLists* xl = nullptr) {
  const int C = g.C, Cx = x.C;
  const bool forced = Cx > C;
  out->plain_us = forced ? 0.0 : envelope_model_us(nblk, plain_last, nullptr);
  if (!forced && (C < 8 || !gaps_ok)) return false;
  // cameras of every point, ascending
  std::vector<int> pstart_s, pcam_s, xstart_s, xcam_s;
  if (!gl) point_camera_lists(g, &pstart_s, &pcam_s);
  if (forced && !xl) point_camera_lists(x, &xstart_s, &xcam_s);
  const std::vector<int>& pstart = gl ? gl->start : pstart_s;
  const std::vector<int>& pcam = gl ? gl->cam : pcam_s;
  const std::vector<int>& xstart = forced ? (xl ? xl->start : xstart_s) : pstart;
  const std::vector<int>& xcam = forced ? (xl ? xl->cam : xcam_s) : pcam;
  const int xP = (int)xstart.size() - 1;  // (== x.P)
  int max_jump = 0;
  for (int q = 0; q < g.P; ++q)
    for (int k = pstart[q] + 1; k < pstart[q + 1]; ++k) max_jump = std::max(max_jump, pcam[k] - pcam[k - 1]);
  bool found = false;
  double best = mode == SK_BORDER_ON ? std::numeric_limits<double>::max() : 0.9 * out->plain_us;
  // one candidate: the real cameras marked in `mark` (nb of them) and every pseudo-camera behind the band
  auto candidate = [&](std::vector<char>& mark, int nb, int gap, int variant, BorderChoice* cand) {
    mark.resize(Cx, 1);
    // first band camera each border camera couples with (through any of its points): the border is ordered so that the
    // cameras reached first come LAST — a column's tail rows are a suffix of the matrix
    std::vector<int> band_id(Cx, -1);
    int Cb = 0;
    for (int c = 0; c < Cx; ++c) if (!mark[c]) band_id[c] = Cb++;
    std::vector<int> first_band(Cx, Cx);
    for (int q = 0; q < xP; ++q) {
      int mn = Cx;
      for (int k = xstart[q]; k < xstart[q + 1]; ++k) if (!mark[xcam[k]]) { mn = band_id[xcam[k]]; break; }
      for (int k = xstart[q]; k < xstart[q + 1]; ++k) if (mark[xcam[k]]) first_band[xcam[k]] = std::min(first_band[xcam[k]], mn);
    }
    std::vector<int> border;
    for (int c = 0; c < Cx; ++c) if (mark[c]) border.push_back(c);
    std::stable_sort(border.begin(), border.end(), [&](int a, int b) { return first_band[a] > first_band[b]; });
    cand->new_id = band_id;
    for (size_t k = 0; k < border.size(); ++k) cand->new_id[border[k]] = Cb + (int)k;
    std::vector<int> first_col;
    if (xl || (gl && !forced)) first_cols_from_lists(xstart, xcam, cand->new_id, nblk, &first_col);  // (the same minima as envelope_of_order's, point by point)
    else (void)envelope_of_order(*x.ocam, *x.opt, cand->new_id, Cx, x.P, nblk, &first_col);
    cholesky_envelope_bordered(first_col, (9 * Cb) / 128, &cand->last, &cand->tail);
    cand->model_us = envelope_model_us(nblk, cand->last, cand->tail.data());
    cand->border_cams = nb; cand->gap = gap; cand->variant = variant;
    mark.resize(C);
  };
  if (forced) {
    std::vector<char> mark(C, 0);
    BorderChoice cand;
    candidate(mark, 0, 0, 0, &cand);
    out->plain_us = cand.model_us;
    cand.plain_us = cand.model_us;
    *out = cand; found = true;
    best = mode == SK_BORDER_ON ? cand.model_us : 0.9 * cand.model_us;  // (loop-closure cameras on top of the pseudo-cameras: when the model gains another 10 %)
  }
  // the candidates (gap, variant): their marks first — cheap, and a candidate whose marks repeat the one before it is dropped — then their
  // envelopes side by side on host threads (plan_parallel_for), then the choice, in the candidates' order
  struct GapCand { int gap, variant, nb; std::vector<char> mark; BorderChoice bc; };
  std::vector<GapCand> gc, all;
  for (int gap = 4; gaps_ok && C >= 8 && gap < C && gap < max_jump; gap *= 2)
    for (int variant = 0; variant < 2; ++variant) all.push_back(GapCand{gap, variant, 0, std::vector<char>(), BorderChoice()});
  plan_parallel_for((int)all.size(), [&](int ai) {  // (a pass over every point's list per candidate: side by side)
    GapCand& c = all[(size_t)ai];
    const int gap = c.gap;
    std::vector<char>& mark = c.mark;
    mark.assign((size_t)C, 0);
    int nb = 0;
    for (int q = 0; q < g.P; ++q) {
      const int a = pstart[q], e = pstart[q + 1];
      if (c.variant == 0) {  // everything behind the first jump
        int k = a + 1;
        while (k < e && pcam[k] - pcam[k - 1] <= gap) ++k;
        for (; k < e; ++k) if (!mark[pcam[k]]) { mark[pcam[k]] = 1; ++nb; }
      } else {             // everything before the last jump
        int k = e - 1;
        while (k > a && pcam[k] - pcam[k - 1] <= gap) --k;
        for (int i = a; i < k; ++i) if (!mark[pcam[i]]) { mark[pcam[i]] = 1; ++nb; }
      }
    }
    c.nb = nb;
  });
  {
    std::vector<char> prev_mark;
    for (GapCand& c : all) {
      if (c.nb == 0 || c.nb > C / 4 || C - c.nb < 4) continue;   // (a border that wide is no border: its dense system would be the factorisation)
      if (c.mark == prev_mark) continue;
      prev_mark = c.mark;
      gc.push_back(std::move(c));
    }
  }
  plan_parallel_for((int)gc.size(), [&](int i) { candidate(gc[(size_t)i].mark, gc[(size_t)i].nb, gc[(size_t)i].gap, gc[(size_t)i].variant, &gc[(size_t)i].bc); });
  for (GapCand& c : gc) {
    c.bc.plain_us = out->plain_us;
    if (c.bc.model_us < best) { best = c.bc.model_us; *out = c.bc; found = true; }
  }
  return found;
}

// The order of the cameras inside the reduced system as setup() takes it: the candidate with the fewest trailing-update flops,
// or a bordered variant of one of the candidates when the chain model prefers it.  From host data alone.
// g: the eliminated points' observations over the real cameras; x: the reduced system's structure (== g without retained points), whose
// pseudo-cameras always go to the border.  npad: padded order of the reduced system (x.C cameras).
static CameraOrderPlan plan_camera_order(const Problem& p, const std::vector<int>& cam_block, const CamGraph& g, const CamGraph& x,
                                         int npad, bool with_memory_order, bool border_ok, int border_mode) {
  CameraOrderPlan out;
  const int nblk = npad / 128, C = g.C, Cx = x.C;
  const bool forced = Cx > C;
  const std::vector<std::vector<int>> cand = camera_order_candidates(p, cam_block, *g.ocam, *g.opt, C, g.P, with_memory_order);
  std::vector<int> best_env;
  int best_k = 0;
  double best = 0.0;
  if (!forced) choose_camera_order(cand, *g.ocam, *g.opt, C, g.P, npad, &best_k, &best_env, &best);
  if (border_ok || forced) {
    // every candidate order may hide a band behind a few revisits: the border is tried on each, the chain model compares
    double best_us = 0.0;
    // (the candidates' borders side by side on host threads; which one is taken: in the candidates' order, below)
    std::vector<BorderChoice> bcs(cand.size());
    std::vector<char> bc_ok(cand.size(), 0);
    // the cameras of every point once, in the numbering the graphs come in: a candidate order's lists are these, renumbered and sorted again
    // point by point (no counting sort over every observation per candidate)
    PointLists gl0, xl0;
    point_camera_lists(g, &gl0.start, &gl0.cam);
    if (forced) point_camera_lists(x, &xl0.start, &xl0.cam);
    auto renumbered = [&](const PointLists& l0, const std::vector<int>& id, PointLists* out) {
      out->start = l0.start;
      out->cam.resize(l0.cam.size());
      for (size_t i = 0; i < l0.cam.size(); ++i) { const int c = l0.cam[i]; out->cam[i] = c < C ? id[(size_t)c] : c; }  // (pseudo-cameras keep their places behind the real ones)
      const int P = (int)l0.start.size() - 1;
      for (int q = 0; q < P; ++q) std::sort(out->cam.begin() + l0.start[(size_t)q], out->cam.begin() + l0.start[(size_t)q + 1]);
    };
    plan_parallel_for((int)cand.size(), [&](int ki) {
      const size_t k = (size_t)ki;
      if (k == 1 && !with_memory_order) return;  // (the slot repeats candidate 0)
      PointLists glk, xlk;
      renumbered(gl0, cand[k], &glk);
      if (forced) renumbered(xl0, cand[k], &xlk);
      const CamGraph gk{nullptr, nullptr, C, g.P}, xk{nullptr, nullptr, Cx, x.P};  // (choose_border reads the lists alone)
      std::vector<int> plain;
      if (!forced) plain = (int)k == best_k ? best_env : envelope_of_order(*g.ocam, *g.opt, cand[k], C, g.P, nblk);
      bc_ok[k] = choose_border(gk, xk, nblk, plain, border_mode, border_ok, &bcs[k], &glk, forced ? &xlk : nullptr) ? 1 : 0;
    });
    for (size_t k = 0; k < cand.size(); ++k) {
      if (k == 1 && !with_memory_order) continue;
      if (!bc_ok[k]) continue;
      const BorderChoice& bc = bcs[k];
      if (!out.bordered || bc.model_us < best_us) {
        best_us = bc.model_us; out.bordered = true; out.candidate = (int)k;
        out.border = bc;
        for (int c = 0; c < Cx; ++c) out.border.new_id[c] = bc.new_id[c < C ? cand[k][c] : c];  // first-appearance numbering -> final numbering
      }
    }
    // (against the envelope of the order that would be used otherwise)
    if (!forced) {
      const double plain_us = envelope_model_us(nblk, best_env, nullptr);
      if (out.bordered && border_mode != SK_BORDER_ON && out.border.model_us >= 0.9 * plain_us) out.bordered = false;
    }
  }
  if (!forced) { out.border.plain_us = envelope_model_us(nblk, best_env, nullptr); out.plain_id = cand[best_k]; }
  out.candidates = cand;
  if (out.bordered) {
    out.id = out.border.new_id; out.last = out.border.last; out.tail = out.border.tail;
    out.flops = cholesky_syrk_flops(npad, 1, out.last.data(), false, nullptr, -1, 1, out.tail.data());
    out.model_us = out.border.model_us;
  } else {
    out.id = cand[best_k]; out.last = best_env; out.candidate = best_k; out.flops = best;
    out.model_us = out.border.plain_us;
  }
  return out;
}

// ---- retained points (round 4): the few points with the longest tracks stay IN the reduced system ---------------------------------
// The Schur complement of a point seen by k cameras is a dense k x k square of camera blocks.  A landmark that stays in view for
// hundreds of frames — five such points among the 156 502 of the Ladybug-shaped problem — sets the height of the block envelope for
// every block column it spans (there: 25-55 block rows where the other points need 8-19; 166 of the 176 GFlop of the
// factorisation).  Such a point is not eliminated: its three coordinates stay in the reduced system as three more rows, behind the
// cameras — [S W; W^T T] (y_c; y_p) = (g_c; g_p) with S, g_c formed from the other points alone, W = F^T E (9 x 3 per observation),
// T = sum E^T E + D_p^2 — which is a BORDER in the sense of the loop-closure cameras above: rows that are active from the first
// camera that sees the point.  Three retained points share a pseudo-camera (nine rows), so that every layout of the reduced
// system — the bordered envelope, the fronts of a dissection — takes them as they take cameras.  The step is the same linear
// system's solution (EX/SimpleBundleAdjuster.scala:147-152: the result of DENSE_SCHUR does not depend on which unknowns were
// eliminated first); tests hold it against the all-eliminated order and the oracle.
// Which points: by the span of their cameras in the banded numbering, widest first, in steps of 3, 6, 12, ... as long as the chain
// model of the bordered envelope improves; taken when it predicts 10 % less than the plan without them (SK_RETAINED_ON: the best
// count whatever the model says).
struct RetainedChoice {
  std::vector<int> points;   // point ids, three to a pseudo-camera, pseudo-cameras in index order
  double model_us = 0.0;
};
// the two graphs of a problem whose points `points` (slot s -> pseudo-camera C + s / 3) are retained
static RetainedGraphs retained_graphs(const std::vector<int>& ocam, const std::vector<int>& opt, int C, int P, const std::vector<int>& points) {
  RetainedGraphs r;
  std::vector<int> slot(P, -1);
  for (size_t s = 0; s < points.size(); ++s) slot[points[s]] = (int)s;
  r.Cx = C + ((int)points.size() + 2) / 3; r.Px = P;
  r.ocam_g.reserve(ocam.size()); r.opt_g.reserve(ocam.size()); r.ocam_x.reserve(ocam.size() + ocam.size() / 8); r.opt_x.reserve(ocam.size() + ocam.size() / 8);
  for (size_t b = 0; b < ocam.size(); ++b) {
    const int s = slot[opt[b]];
    if (s < 0) { r.ocam_g.push_back(ocam[b]); r.opt_g.push_back(opt[b]); r.ocam_x.push_back(ocam[b]); r.opt_x.push_back(opt[b]); continue; }
    r.ocam_x.push_back(ocam[b]); r.opt_x.push_back(r.Px);
    r.ocam_x.push_back(C + s / 3); r.opt_x.push_back(r.Px);
    ++r.Px;
  }
  return r;
}
// ocam: cameras in the banded numbering (the best candidate order, no border).  base_us: the model of the plan without retained points.
// families: bit 0 — the widest tracks by span and by number of observations, in doubling counts; bit 1 — the tracks of loop closures (below)
static RetainedChoice choose_retained_points(const std::vector<int>& ocam, const std::vector<int>& opt, int C, int P, int mode, int max_points, bool gaps_ok,
                                             double base_us, int families = 3) {
  RetainedChoice out;
  if (mode == SK_RETAINED_OFF) return out;
  if (mode == SK_RETAINED_AUTO && (C < 64 || (9 * C + 128) / 128 < 16)) return out;  // (a reduced system of a few blocks: nothing to gain)
  std::vector<int> cmin(P, C), cmax(P, -1), cnt(P, 0);
  for (size_t b = 0; b < ocam.size(); ++b) { cmin[opt[b]] = std::min(cmin[opt[b]], ocam[b]); cmax[opt[b]] = std::max(cmax[opt[b]], ocam[b]); cnt[opt[b]]++; }
  // (a point with two residual blocks on one camera is never retained: the rows of a retained point have one writer per block)
  // (the cameras of every point, ascending — formed once: the candidates' graphs are derived from these lists, below — and a camera that
  // comes twice in a point's list is two residual blocks on one pair)
  PointLists base;
  { const CamGraph g0{&ocam, &opt, C, P}; point_camera_lists(g0, &base.start, &base.cam); }
  std::vector<char> twice(P, 0);
  for (int q = 0; q < P; ++q)
    for (int k = base.start[(size_t)q] + 1; k < base.start[(size_t)q + 1]; ++k) if (base.cam[(size_t)k] == base.cam[(size_t)k - 1]) twice[(size_t)q] = 1;
  std::vector<int> wide;
  for (int q = 0; q < P; ++q) if (cnt[q] >= 2 && 9 * (cmax[q] - cmin[q]) >= 128 && !twice[q]) wide.push_back(q);
  const bool exactly = mode == SK_RETAINED_ON && max_points > 0;  // (ON with a count: that many, as far as there are candidates)
  if (max_points <= 0) max_points = 1536;
  max_points = std::min(max_points - max_points % 3, (int)wide.size() - (int)wide.size() % 3);
  double best = mode == SK_RETAINED_ON ? std::numeric_limits<double>::max() : 0.9 * base_us;
  // Two orders of the candidates: by the span of their cameras (whatever widens the envelope: landmarks AND the tracks of loop
  // closures, which a border of retained points can take as well as a border of cameras can), and by the number of their
  // observations (the landmarks alone — the loop closures are then left to the border of cameras, when the problem has both)
  // One candidate set of points -> the chain model of the plan with them retained (a border of their pseudo-cameras, loop-closure cameras on top
  // where that pays).  Memoised, and evaluated a few candidates AHEAD in parallel: the loops below take them in their own order.
  struct Scored { bool ok = false; double model_us = 0.0; };
  std::map<std::vector<int>, Scored> scored;  // (key: the set, sorted)
  // the cameras of every point, once; a candidate's graphs are these lists with the retained points' taken out (g) and, behind them, a point
  // of two cameras — the observation's and the retained point's pseudo-camera — for every observation of a retained point (x: retained_graphs)
  auto lists_with = [&](const std::vector<int>& pts, PointLists* l, int* Cx, int* Px) {
    std::vector<int> slot((size_t)P, -1);
    for (size_t k = 0; k < pts.size(); ++k) slot[(size_t)pts[k]] = (int)k;
    int extra = 0;
    for (int q : pts) extra += base.start[(size_t)q + 1] - base.start[(size_t)q];
    *Cx = C + ((int)pts.size() + 2) / 3; *Px = P + extra;
    l->start.assign((size_t)*Px + 1, 0);
    l->cam.clear(); l->cam.reserve(base.cam.size() + (size_t)extra);
    for (int q = 0; q < P; ++q) {
      if (slot[(size_t)q] < 0) l->cam.insert(l->cam.end(), base.cam.begin() + base.start[(size_t)q], base.cam.begin() + base.start[(size_t)q + 1]);
      l->start[(size_t)q + 1] = (int)l->cam.size();
    }
    int np = P;
    for (int q : pts)
      for (int k = base.start[(size_t)q]; k < base.start[(size_t)q + 1]; ++k) {
        l->cam.push_back(base.cam[(size_t)k]); l->cam.push_back(C + slot[(size_t)q] / 3);
        l->start[(size_t)++np] = (int)l->cam.size();
      }
  };
  auto key_of = [](const std::vector<int>& pts) { std::vector<int> k(pts); std::sort(k.begin(), k.end()); return k; };
  auto score_ahead = [&](const std::vector<std::vector<int>>& sets) {
    std::vector<const std::vector<int>*> todo;
    std::vector<std::vector<int>> keys;
    for (const std::vector<int>& pts : sets) {
      std::vector<int> k = key_of(pts);
      if (scored.count(k) || std::find(keys.begin(), keys.end(), k) != keys.end()) continue;
      keys.push_back(std::move(k)); todo.push_back(&pts);
    }
    std::vector<Scored> res(todo.size());
    plan_parallel_for((int)todo.size(), [&](int i) {
      PointLists l;
      int Cx = 0, Px = 0;
      lists_with(*todo[i], &l, &Cx, &Px);
      const int nblk = (9 * Cx + 1 + 127) / 128;
      BorderChoice bc;
      // (g's lists are the first P of x's: one object serves as both)
      res[i].ok = choose_border(CamGraph{nullptr, nullptr, C, P}, CamGraph{nullptr, nullptr, Cx, Px}, nblk, {}, SK_BORDER_AUTO, gaps_ok, &bc, &l, &l);
      res[i].model_us = bc.model_us;
    });
    for (size_t i = 0; i < todo.size(); ++i) scored[keys[i]] = res[i];
  };
  auto score = [&](const std::vector<int>& pts) { std::vector<int> k = key_of(pts); if (!scored.count(k)) score_ahead({pts}); return scored[k]; };
  // the candidate sets of one order of the wide tracks, in doubling counts
  auto sets_of_order = [&](std::vector<std::vector<int>>* sets) {
    for (int R = exactly ? std::max(3, max_points) : 3; R <= max_points; R = R < 6 ? 6 : 2 * R) {
      std::vector<int> pts(wide.begin(), wide.begin() + R);
      // pseudo-cameras in the order the border wants them: the points reached first come last
      std::sort(pts.begin(), pts.end(), [&](int a, int b) { return cmin[a] != cmin[b] ? cmin[a] > cmin[b] : a < b; });
      sets->push_back(std::move(pts));
    }
  };
  std::vector<std::vector<int>> seen_sets;
  for (int by_count = 0; (families & 1) && by_count < (exactly ? 1 : 2); ++by_count) {
    std::sort(wide.begin(), wide.end(), [&](int a, int b) {
      const int sa = by_count ? cnt[a] : cmax[a] - cmin[a], sb = by_count ? cnt[b] : cmax[b] - cmin[b];
      return sa != sb ? sa > sb : a < b;
    });
    double best_here = std::numeric_limits<double>::max();
    std::vector<std::vector<int>> sets;
    sets_of_order(&sets);
    for (size_t si = 0; si < sets.size(); ++si) {
      const std::vector<int>& pts = sets[si];
      const int R = (int)pts.size();
      // (the same set of points under the other order — the landmarks are usually the widest tracks by either measure — is not planned twice:
      // a candidate of Venice-1778's size costs most of a second)
      { std::vector<int> key = key_of(pts); if (std::find(seen_sets.begin(), seen_sets.end(), key) != seen_sets.end()) continue; seen_sets.push_back(key); }
      // (this candidate and the next three: the loop usually ends — 25 % past its best — within a few counts of where it is)
      if (!scored.count(key_of(pts))) score_ahead(std::vector<std::vector<int>>(sets.begin() + (long)si, sets.begin() + (long)std::min(sets.size(), si + 4)));
      const Scored sc = score(pts);
      if (!sc.ok) continue;
      struct { double model_us; } bc{sc.model_us};
      if (dev_knobs().debug_envelope) std::fprintf(stderr, "[skeres_amd] retained candidates: the %d widest tracks by %s: chain model %.0f us (best so far %.0f, base %.0f)\n", R, by_count ? "observations" : "span", bc.model_us, best, base_us);
      // (a LARGER set has to beat a smaller one by 1 %: the model is no finer than that, and every retained point is three more rows that
      // every later column carries.  Ladybug-1723, one box, Cholesky phase per iteration with 6 / 12 / 24 points retained: 4.06 / 3.82 /
      // 3.92 ms, where the model says 5362 / 5304 / 5303 us — profiles/r05_retained_count_ab.txt)
      if (bc.model_us < (out.points.empty() || pts.size() <= out.points.size() ? 1.0 : 0.99) * best) { best = bc.model_us; out.points = pts; out.model_us = bc.model_us; }
      if (bc.model_us > 1.25 * best_here) break;  // (well past the best count of this order: more border rows only cost)
      best_here = std::min(best_here, bc.model_us);
    }
  }
  // A third family (round 5): the tracks of LOOP CLOSURES — points whose ascending camera list has a jump of more than `gap` cameras, the
  // test choose_border applies to cameras — ALL of them, at their exact number, then the widest of the other tracks behind them.  The
  // doubling counts above cannot find this set: 0.5 % of the Ladybug-shaped problem's tracks seen from two distant windows are 782 points,
  // whose rows keep the envelope full until the last one of them is retained (768 points: nothing gained) and cost twice their rows at
  // the next count (1536); retained exactly — 19 block rows of border — the band keeps its own width.
  if (!exactly && C >= 64 && (families & 2)) {
    const std::vector<int>& pstart = base.start;  // (the cameras of every point, ascending: formed above)
    const std::vector<int>& pcam = base.cam;
    std::vector<int> jump(P, 0);
    int max_jump = 0;
    for (int q = 0; q < P; ++q) {
      for (int k = pstart[q] + 1; k < pstart[q + 1]; ++k) jump[q] = std::max(jump[q], pcam[k] - pcam[k - 1]);
      max_jump = std::max(max_jump, jump[q]);
    }
    std::vector<int> by_cnt(wide);
    std::sort(by_cnt.begin(), by_cnt.end(), [&](int a, int b) { return cnt[a] != cnt[b] ? cnt[a] > cnt[b] : a < b; });
    size_t prev_size = 0;
    for (int gap = 16; gap < C && gap < max_jump; gap *= 2) {
      std::vector<int> closing;
      for (int q : wide) if (jump[q] > gap) closing.push_back(q);
      if (closing.empty()) break;
      if (dev_knobs().debug_envelope) std::fprintf(stderr, "[skeres_amd] retained candidates: %zu wide tracks with a jump of more than %d cameras (max_points %d)\n", closing.size(), gap, max_points);
      if ((int)closing.size() > max_points || closing.size() == prev_size) continue;
      prev_size = closing.size();
      std::vector<char> in(P, 0);
      for (int q : closing) in[q] = 1;
      std::vector<std::vector<int>> both;
      for (int more : {12, 48}) {  // ... and a few of the landmarks on top (by their number of observations)
        std::vector<int> pts(closing);
        int added = 0;
        for (size_t k = 0; k < by_cnt.size() && (added < more || pts.size() % 3 != 0); ++k)
          if (!in[by_cnt[k]]) { pts.push_back(by_cnt[k]); ++added; }
        if (pts.size() % 3 != 0 || (int)pts.size() > max_points + 2) { both.emplace_back(); continue; }
        std::sort(pts.begin(), pts.end(), [&](int a, int b) { return cmin[a] != cmin[b] ? cmin[a] > cmin[b] : a < b; });
        both.push_back(std::move(pts));
      }
      { std::vector<std::vector<int>> ahead; for (const auto& v : both) if (!v.empty()) ahead.push_back(v); score_ahead(ahead); }
      for (int mi = 0; mi < 2; ++mi) {
        const int more = mi == 0 ? 12 : 48;
        const std::vector<int>& pts = both[mi];
        if (pts.empty()) continue;
        const Scored sc = score(pts);
        if (!sc.ok) continue;
        struct { double model_us; } bc{sc.model_us};
        if (dev_knobs().debug_envelope) std::fprintf(stderr, "[skeres_amd] retained candidates: gap %d + %d landmarks = %zu points: chain model %.0f us (best so far %.0f, base %.0f)\n", gap, more, pts.size(), bc.model_us, best, base_us);
        if (bc.model_us < (out.points.empty() || pts.size() <= out.points.size() ? 1.0 : 0.99) * best) { best = bc.model_us; out.points = pts; out.model_us = bc.model_us; }
      }
    }
  }
  return out;
}

// The layout of the reduced system as setup() takes it: the camera order (with its border of loop-closure cameras), and — when
// retained_mode allows and the chain model agrees — the retained points with their pseudo-cameras.  From host data alone.
ReducedSystemPlan plan_reduced_system(const Problem& p, const std::vector<int>& cam_block, const std::vector<int>& ocam, const std::vector<int>& opt, int C, int P,
                                      bool with_memory_order, bool border_ok, int border_mode, int retained_mode, int retained_max) {
  ReducedSystemPlan out;
  const CamGraph g0{&ocam, &opt, C, P};
  const int npad = ((9 * C + 1 + 127) / 128) * 128;
  out.order = plan_camera_order(p, cam_block, g0, g0, npad, with_memory_order, border_ok, border_mode);
  out.without_us = out.order.model_us;
  if (retained_mode == SK_RETAINED_OFF) return out;
  // The retained points are chosen on a banded numbering of the cameras: the best candidate order as it stands — and, round 5, the
  // other candidates too: with loop closures all over the sequence the order with the fewest flops is a reverse Cuthill-McKee one in
  // which every track has jumps, and the tracks that CLOSE loops (choose_retained_points, third family) can only be told from the
  // others in the capture order (memory order / first appearance).  The chain model of the whole plan compares.
  std::vector<std::vector<int>> bases;
  std::vector<int> families;
  const std::vector<std::vector<int>> cands = out.order.candidates;  // (of the same graph: formed once)
  bases.push_back(out.order.plain_id);
  families.push_back(1 | ((out.order.plain_id == cands[0] || out.order.plain_id == cands[1]) ? 2 : 0));
  for (int k = 0; k < 2; ++k)  // (the capture orders: first appearance, memory order)
    if (std::find(bases.begin(), bases.end(), cands[k]) == bases.end()) { bases.push_back(cands[k]); families.push_back(2); }
  std::vector<std::vector<int>> tried;
  const CameraOrderPlan without = out.order;
  for (size_t bi = 0; bi < bases.size(); ++bi) {
    const std::vector<int>& base = bases[bi];
    std::vector<int> oc(ocam.size());
    for (size_t b = 0; b < ocam.size(); ++b) oc[b] = base[ocam[b]];
    const RetainedChoice rc = choose_retained_points(oc, opt, C, P, retained_mode, retained_max, border_ok, without.model_us, families[bi]);
    if (rc.points.empty()) continue;
    std::vector<int> key(rc.points);
    std::sort(key.begin(), key.end());
    if (std::find(tried.begin(), tried.end(), key) != tried.end()) continue;
    tried.push_back(key);
    RetainedGraphs rg = retained_graphs(ocam, opt, C, P, rc.points);
    const int npadx = ((9 * rg.Cx + 1 + 127) / 128) * 128;
    CameraOrderPlan px = plan_camera_order(p, cam_block, rg.g(C, P), rg.x(), npadx, with_memory_order, border_ok, border_mode);
    const bool first = out.retained.empty();
    if (first ? (retained_mode == SK_RETAINED_ON || px.model_us < 0.9 * without.model_us) : px.model_us < out.order.model_us) {
      out.order = std::move(px); out.retained = rc.points; out.graphs = std::move(rg);
    }
    if (retained_mode == SK_RETAINED_ON && retained_max > 0) break;  // (an exact count: the widest tracks of the plan's own order)
  }
  return out;
}

// ---- where the camera sequence is cut ------------------------------------------------------------------------------------
static std::vector<int> identity_order(int n) { std::vector<int> e(n); std::iota(e.begin(), e.end(), 0); return e; }

bool band_is_chain_bound(const BandStructure& s) {
  if (s.border_members <= 0 || s.env->empty() || s.env_tail->empty()) return false;
  const BlockEnvelope env(s.nblk, s.env->data(), s.env_tail->data());
  bool bound = true;
  for (int c = 0; bound && c < s.nblk - 1 && c < (9 * (s.C - s.border_members)) / 128; ++c) bound = chain_bound(env.height(c));
  return bound;
}

// forced (tests, small problems): cut the sequence of C cameras at its middle camera wherever that leaves a tail
static void force_middle_cut(const std::vector<int>& ocam, const std::vector<int>& opt, int C, int P, Dissection* ds) {
  std::vector<int> cmin(P, C), cmax(P, -1);
  for (size_t b = 0; b < ocam.size(); ++b) { cmin[opt[b]] = std::min(cmin[opt[b]], ocam[b]); cmax[opt[b]] = std::max(cmax[opt[b]], ocam[b]); }
  for (int a = C / 2; a >= 1 && ds->a == 0; --a) {
    int b = a;
    for (int q = 0; q < P; ++q) if (cmin[q] < a) b = std::max(b, cmax[q] + 1);
    if (b < C) { ds->a = a; ds->b = b; }
  }
}

// One pass of setup()'s cut loop, for a sequence that may be dissected.  Several ranks (f.multi, not the two-segment trial): the
// SEGMENTED distribution — every rank's device eliminates one segment — when the model of the chains predicts a gain (or when asked
// for).  One device, or the two-segment trial of a world with retained points: a border — the cameras of loop closures, the
// pseudo-cameras of retained points — joins the ONE separator, which both fronts border on, and the band in front of it is what is cut.
CutPlan plan_cuts(const BandStructure& s, const CutFlags& f, CutModel* model) {
  CutPlan out;
  const std::vector<int>& ocam = *s.ocam;
  const std::vector<int>& opt = *s.opt;
  const int C = s.C, P = s.P, nblk = s.nblk;
  const std::vector<int>& env_tail = *s.env_tail;
  const bool pseudo_border = f.pseudo_border, two_seg_try = f.two_seg_try, lockstep_cut = f.lockstep_cut;
  const bool segmented_mode = f.distribution_mode == SK_DISTRIBUTION_SEGMENTED;
  const int Cband = C - (pseudo_border ? s.border_members : 0);
  int max_seg = f.world;
  if (f.max_segments >= 2) max_seg = std::min(max_seg, f.max_segments);  // (sk_options_set_max_segments)
  if (f.multi && !two_seg_try) {
    std::vector<int> first_col;
    (void)envelope_of_order(ocam, opt, identity_order(C), C, P, nblk, &first_col);
    const Segments sg = choose_segments(ocam, opt, C, P, nblk, *s.env, first_col, max_seg, segmented_mode, f.world);
    out.a = sg.a; out.b = sg.b;
    model->t_plain = sg.t_plain; model->t_model = sg.t_model;
    for (int k = 0; k < 9; ++k) model->model_us[k] = sg.model_us[k];
    return out;
  }
  Dissection ds;
  std::vector<int> first_col, many_cut_a, many_cut_b;
  double dissect_t_model_many = 0.0;
  // what is cut: the cameras' band — with a border, the band cameras under the points that are eliminated (the border's cameras
  // and what they see belong to the separator whatever the cut)
  std::vector<int> cut_ocam, cut_opt;
  if (pseudo_border) {
    const std::vector<int>& so = s.pseudo_cams > 0 ? *s.band_ocam : ocam;
    const std::vector<int>& sp = s.pseudo_cams > 0 ? *s.band_opt : opt;
    for (size_t b = 0; b < so.size(); ++b) if (so[b] < Cband) { cut_ocam.push_back(so[b]); cut_opt.push_back(sp[b]); }
  }
  const std::vector<int>& docam = pseudo_border ? cut_ocam : ocam;
  const std::vector<int>& dopt = pseudo_border ? cut_opt : opt;
  const int dnblk = pseudo_border ? (9 * Cband + 1 + 127) / 128 : nblk;
  const std::vector<int> band_env = envelope_of_order(docam, dopt, identity_order(Cband), Cband, P, dnblk, &first_col);
  const std::vector<int>& denv = pseudo_border ? band_env : *s.env;
  // (the border's rows that a band column reaches on top of its run: the tail profile of the bordered envelope)
  std::vector<int> extra_fwd, extra_bwd_col;
  const int extra_bwd = 0;
  if (pseudo_border) {
    extra_fwd.assign(dnblk, 0);
    for (int c = 0; c < dnblk && c < (int)env_tail.size(); ++c) extra_fwd[c] = std::max(0, nblk - 1 - std::max(env_tail[c], c + 1));
    // (the tail front reaches the border's rows in another order; counting all of them in every one of its columns moved the cut of
    // Venice-1778 to a worse place — Cholesky phase 5.26 against 4.94 ms — and counting none made the model of a border of 800 retained
    // points 40 % too low (round 5: 6.1 against 10.1 ms with the tracks of scattered loop closures retained).  Counted per column: a
    // member of the border is active in the tail's columns from the LAST band camera that sees it back to the cut.)
    const std::vector<int>& xo = s.struct_ocam->empty() ? ocam : *s.struct_ocam;
    const std::vector<int>& xp = s.struct_ocam->empty() ? opt : *s.struct_opt;
    const int xP = s.struct_ocam->empty() ? P : s.struct_P;
    std::vector<int> pmax(xP, -1), reach_max(C - Cband, -1);
    for (size_t b = 0; b < xo.size(); ++b) if (xo[b] < Cband) pmax[xp[b]] = std::max(pmax[xp[b]], xo[b]);
    for (size_t b = 0; b < xo.size(); ++b) if (xo[b] >= Cband) reach_max[xo[b] - Cband] = std::max(reach_max[xo[b] - Cband], pmax[xp[b]]);
    std::vector<int> active(dnblk + 1, 0);  // members whose last band camera lies in block column c or behind it
    for (int m : reach_max) if (m >= 0) active[std::min(dnblk - 1, (9 * m) / 128)]++;
    for (int c = dnblk - 2; c >= 0; --c) active[c] += active[c + 1];
    extra_bwd_col.assign(dnblk, 0);
    for (int c = 0; c < dnblk; ++c) extra_bwd_col[c] = (9 * active[c] + 127) / 128;
  }
  const std::vector<int>* fwd_p = pseudo_border ? &extra_fwd : nullptr;
  const std::vector<int>* bwd_p = pseudo_border ? &extra_bwd_col : nullptr;
  const int members = C - Cband;
  const std::vector<int> band_reach = camera_reach(docam, dopt, Cband, P);  // (once for every cut planned on this sequence, below)
  // one device: the lock-step schedule and its own cut
  ds = choose_dissection(docam, dopt, Cband, P, dnblk, denv, first_col, lockstep_cut || two_seg_try, lockstep_cut, members, fwd_p, extra_bwd, bwd_p, &band_reach);
  if (two_seg_try) {
    // two devices, a chain each, against ONE device with the two fronts in lock-step (what a replicating rank would run): + the
    // all-reduce of the separator's system (its lower triangle over one xGMI link per direction)
    const Dissection one = choose_dissection(docam, dopt, Cband, P, dnblk, denv, first_col, true, true, members, fwd_p, extra_bwd, bwd_p, &band_reach);
    const double one_us = one.a > 0 ? one.t_dissected : one.t_plain;
    const double E = ds.a > 0 ? (9.0 * (ds.b - ds.a + members) + 1.0 + 127.0) / 128.0 : 0.0;
    // (+ the three small collectives of a segmented iteration — column norms and gradient, two tables of scalars — at the cost of a
    // latency-bound all-reduce each)
    const double allreduce_us = kAllreduceUs + 3.0 * kSmallAllreduceUs + allreduce_triangle_us(E, f.world);
    // (the phases that shard with the points — two ranks take half of them each)
    const double shard_us = 1e6 * shardable_work_s(pair_entries(opt, P), (double)opt.size());
    model->model_us[1] = one_us; model->model_us[2] = ds.a > 0 ? ds.t_dissected + allreduce_us : 0.0;
    if (dev_knobs().debug_segments) std::fprintf(stderr, "[skeres_amd] two segments with %d border members in the separator: %.0f us + all-reduce %.0f us against %.0f us on one device\n",
                                                 s.border_members, ds.t_dissected, allreduce_us, one_us);
    if (ds.a > 0 && !segmented_mode && ds.t_dissected + allreduce_us + 0.5 * shard_us >= 0.9 * (one_us + shard_us)) ds.a = ds.b = 0;
    // ... and MORE than two segments, a device each: every segment's front has the members' rows in its border, the root is the
    // separators' block-tridiagonal system bordered by the members (choose_segments; every rank factors it)
    if (max_seg > 2) {
      const Segments sg = choose_segments(docam, dopt, Cband, P, dnblk, denv, first_col, max_seg, segmented_mode, f.world, members, fwd_p, bwd_p, &band_reach);
      for (int k = 3; k < 9; ++k) model->model_us[k] = sg.model_us[k];
      const int Rn = (int)sg.a.size() + 1;
      const double two_us = ds.a > 0 ? ds.t_dissected + allreduce_us + 0.5 * shard_us : 1e300;
      if (Rn > 2 && (segmented_mode || (sg.t_model + shard_us / Rn < 0.95 * two_us && sg.t_model + shard_us / Rn < 0.9 * (one_us + shard_us)))) {
        if (dev_knobs().debug_segments) std::fprintf(stderr, "[skeres_amd] %d segments with %d border members in the root: %.0f us against %.0f us in two\n", Rn, s.border_members, sg.t_model, two_us);
        many_cut_a = sg.a; many_cut_b = sg.b;
        dissect_t_model_many = sg.t_model;
      }
    }
  }
  // (two resident servers per factorisation: the fifth such solver alive on a device stays undissected — the caller's claim)
  out.needs_pair_claim = lockstep_cut && ds.a > 0;
  out.drop_without_claim = out.needs_pair_claim && f.dissect_at < 0;
  // AUTO does not dissect on ONE device: measured on MI355X (profiles/r02_dissection_*), the two chains side by side
  // on one device take longer than one after the other — each alone 5.0 and 3.0 ms, together 10-13 ms; 6.6 ms only under
  // rocprofv3's kernel tracing — so the model's prediction (kept in sk_solver_stat) is not acted upon there.
  if (f.dissection == SK_DISSECTION_AUTO && f.dissect_at < 0 && !lockstep_cut && !two_seg_try) { ds.a = ds.b = 0; }
  if (two_seg_try && segmented_mode && ds.a == 0 && many_cut_a.empty() && Cband >= 6) force_middle_cut(docam, dopt, Cband, P, &ds);  // (the band)
  if (f.dissection == SK_DISSECTION_ON && ds.a == 0 && C >= 6) force_middle_cut(ocam, opt, C, P, &ds);
  if (f.dissect_at >= 0) {  // developer variable SK_DISSECT_AT: head size in cameras (0: no dissection)
    ds.a = f.dissect_at; ds.b = 0;
    if (ds.a > 0 && ds.a < C) {
      ds.b = ds.a;
      std::vector<int> cmin(P, C);
      for (size_t b = 0; b < ocam.size(); ++b) cmin[opt[b]] = std::min(cmin[opt[b]], ocam[b]);
      for (size_t b = 0; b < ocam.size(); ++b) if (cmin[opt[b]] < ds.a) ds.b = std::max(ds.b, ocam[b] + 1);
      if (ds.b >= C) ds.a = ds.b = 0;
    } else ds.a = 0;
  }
  model->t_plain = ds.t_plain; model->t_model = ds.t_dissected;
  if (!two_seg_try) {  // what the chain model predicts for 2 .. 8 devices (sk_solver_stat "model_us_segments_<n>": bench.py prints it beside what it measures)
    const Segments sg = choose_segments(docam, dopt, Cband, P, dnblk, denv, first_col, 8, false, 0, members, fwd_p, bwd_p, &band_reach);
    for (int k = 0; k < 9; ++k) model->model_us[k] = sg.model_us[k];
    if (pseudo_border) {
      // ... and with the border's members (retained points) in the one separator of TWO segments, a device each — what a world of ranks
      // takes when it beats this device's plan by 10 % (the two-segment trial above): "model_us_two_segments_with_members"
      const Dissection two = choose_dissection(docam, dopt, Cband, P, dnblk, denv, first_col, true, false, members, &extra_fwd, extra_bwd, &extra_bwd_col, &band_reach);
      if (two.a > 0) {
        const double E = (9.0 * (two.b - two.a + members) + 1.0 + 127.0) / 128.0;
        model->two_segments_members_us = two.t_dissected + kAllreduceUs + allreduce_triangle_us(E, 2);  // (+ the root's all-reduce over two ranks)
      }
    }
  }
  if (!many_cut_a.empty()) { out.a = many_cut_a; out.b = many_cut_b; model->t_model = dissect_t_model_many; }
  else if (ds.a > 0 && ds.b < Cband) { out.a.push_back(ds.a); out.b.push_back(ds.b); }
  return out;
}

CutNumbering apply_cuts(const CutPlan& cuts, int Cband, int C) {
  CutNumbering n;
  const int R = (int)cuts.a.size() + 1;
  auto lo_of = [&](int sg) { return sg == 0 ? 0 : cuts.b[sg - 1]; };
  auto hi_of = [&](int sg) { return sg + 1 < R ? cuts.a[sg] : Cband; };
  n.seg_off.assign(R + 1, 0);
  for (int sg = 0; sg < R; ++sg) n.seg_off[sg + 1] = n.seg_off[sg] + (hi_of(sg) - lo_of(sg));
  n.fin.resize(C);
  int sep_pos = n.seg_off[R];
  for (int sg = 0; sg < R; ++sg) {
    const int lo = lo_of(sg), hi = hi_of(sg);
    for (int c = lo; c < hi; ++c) n.fin[c] = sg + 1 < R ? n.seg_off[sg] + (c - lo) : n.seg_off[sg] + (hi - 1 - c);
    if (sg + 1 < R) { n.sep_first.push_back(sep_pos); for (int c = cuts.a[sg]; c < cuts.b[sg]; ++c) n.fin[c] = sep_pos++; }
  }
  for (int c = Cband; c < C; ++c) n.fin[c] = sep_pos++;  // the border's members (loop-closure cameras, pseudo-cameras of retained points): the end of the (one) separator
  n.sep_first.push_back(C);
  return n;
}

// ---- this rank's points: a contiguous run of equal sum k^2 (sharded), or (segmented) the points that see a camera of
// its segment — each such point sees only that segment and the separator — plus every other of the points that see the
// separator alone; their observations, point-major; the camera lists; the retained points' tables ----
LocalStructure index_local_structure(const Problem& p, const LocalInputs& in) {
  LocalStructure ls;
  const std::vector<int>& ocam = *in.ocam;
  const std::vector<int>& opt = *in.opt;
  const int Nall = (int)p.rb_functor.size(), C = in.C, P_total = in.P, segments = in.segments, role = in.role;
  std::vector<int>& local_pt = ls.local_pt;
  std::vector<int> local_of(P_total, -1);
  std::vector<int> obs_rank;  // segmented world with retained points: the rank of every observation of a retained point (-1: not one)
  if (in.segmented) {
    const std::vector<int>& seg_off = *in.seg_off;
    std::vector<int> seg_of_cam(C, -1);  // (separator cameras: -1)
    for (int sg = 0; sg < segments; ++sg) for (int c = seg_off[sg]; c < seg_off[sg + 1]; ++c) seg_of_cam[c] = sg;
    std::vector<int> seg_of_pt(P_total, -1);
    // A RETAINED point is seen from every segment its track crosses: its observations are split by camera — those of a segment's cameras
    // to that segment's rank, those of separator cameras to its HOME rank (q mod segments) — and every rank that has any of them keeps a
    // copy of the point.  What is a sum over the point's observations (its column norms, gradient, T = sum E^T E) is summed over the
    // ranks; what is the point's own (D_p^2, the right-hand side's entry, |x_p|^2, |delta_p|^2, the value written back) is the home rank's.
    std::vector<char> is_kept(P_total, 0);
    for (int q : *in.retained_pts) is_kept[q] = 1;
    obs_rank.assign(Nall, -1);  // (kept observations only)
    for (int b = 0; b < Nall; ++b) {
      const int sg = seg_of_cam[ocam[b]];
      if (is_kept[opt[b]]) { obs_rank[b] = sg >= 0 ? sg : opt[b] % segments; continue; }
      if (sg < 0) continue;
      if (seg_of_pt[opt[b]] >= 0 && seg_of_pt[opt[b]] != sg) { ls.error = "internal: a point is seen from two segments of the camera sequence"; return ls; }
      seg_of_pt[opt[b]] = sg;
    }
    std::vector<char> kept_here(P_total, 0);
    for (int b = 0; b < Nall; ++b) if (obs_rank[b] == role) kept_here[opt[b]] = 1;
    std::vector<int> guests;  // copies of retained points whose home is another rank: LAST among the local points (the norms run over the others)
    for (int q = 0; q < P_total; ++q) {
      if (is_kept[q]) {
        const bool home = (q % segments) == role;
        if (home) { local_of[q] = (int)local_pt.size(); local_pt.push_back(q); }
        else if (kept_here[q]) guests.push_back(q);
        continue;
      }
      const bool mine = seg_of_pt[q] == role || (seg_of_pt[q] < 0 && (q % segments) == role);
      if (mine) { local_of[q] = (int)local_pt.size(); local_pt.push_back(q); }
    }
    ls.P_own = (int)local_pt.size();
    for (int q : guests) { local_of[q] = (int)local_pt.size(); local_pt.push_back(q); }
  } else {
    int p_lo = 0, p_hi = P_total;
    if (in.world > 1) {
      std::vector<int> cut;
      bal_partition_points(opt, P_total, in.world, &cut);
      p_lo = cut[in.rank]; p_hi = cut[in.rank + 1];
    }
    local_pt.resize(p_hi - p_lo); std::iota(local_pt.begin(), local_pt.end(), p_lo);
    for (int q = p_lo; q < p_hi; ++q) local_of[q] = q - p_lo;
  }
  const int P = ls.P = (int)local_pt.size();
  if (!in.segmented) ls.P_own = P;
  auto obs_here = [&](int b) { return local_of[opt[b]] >= 0 && (obs_rank.empty() || obs_rank[b] < 0 || obs_rank[b] == role); };
  // local observations, point-major, ascending camera within a point
  std::vector<int>& pt_start = ls.pt_start;
  pt_start.assign(P + 1, 0);
  for (int b = 0; b < Nall; ++b) if (obs_here(b)) pt_start[local_of[opt[b]] + 1]++;
  for (int q = 0; q < P; ++q) pt_start[q + 1] += pt_start[q];
  const int N = ls.N = pt_start[P];
  std::vector<int>& order = ls.order;
  order.resize(N);
  { std::vector<int> fill(pt_start.begin(), pt_start.end() - 1);
    for (int b = 0; b < Nall; ++b) if (obs_here(b)) order[fill[local_of[opt[b]]]++] = b; }
  for (int q = 0; q < P; ++q)
    std::sort(order.begin() + pt_start[q], order.begin() + pt_start[q + 1], [&](int a, int b) { return ocam[a] != ocam[b] ? ocam[a] < ocam[b] : a < b; });
  ls.cam.resize(N); ls.pt.resize(N);
  // captured doubles per observation: (observedX, observedY) of SnavelyReprojectionError, or whatever a recorded functor captures
  for (int b = 0; b < Nall && !ls.tape; ++b) ls.tape = p.tape_of_block(b);
  const int nobs = ls.tape ? ls.tape->num_obs_consts : 2;
  ls.obs.resize((size_t)std::max(1, nobs) * (size_t)N);
  for (int o = 0; o < N; ++o) {
    const int b = order[o];
    ls.cam[o] = ocam[b]; ls.pt[o] = local_of[opt[b]];
    if (p.rb_functor[b] == SK_FUNCTOR_HOST_CALLBACK) {  // no captured doubles on the device: the caller's object holds them
      ls.host_obs.push_back(o); ls.host_cf.push_back(p.rb_cost[b]);
    } else {
      for (int k = 0; k < nobs; ++k) ls.obs[(size_t)k * N + o] = p.consts[p.rb_const_off[b] + k];
    }
  }
  // camera CSR (ascending point because observation order is point-major)
  ls.cam_start.assign(C + 1, 0); ls.cam_obs.resize(N);
  for (int o = 0; o < N; ++o) ls.cam_start[ls.cam[o] + 1]++;
  for (int i = 0; i < C; ++i) ls.cam_start[i + 1] += ls.cam_start[i];
  { std::vector<int> fill(ls.cam_start.begin(), ls.cam_start.end() - 1); for (int o = 0; o < N; ++o) ls.cam_obs[fill[ls.cam[o]]++] = o; }
  ls.slot.resize(N);
  for (int e = 0; e < N; ++e) ls.slot[ls.cam_obs[e]] = e;
  // retained points of this rank: local point, pseudo-camera, slot; their observations
  ls.kept_of_local.assign(P, -1);
  for (size_t k = 0; k < in.retained_pts->size(); ++k) {
    const int q = local_of[(*in.retained_pts)[k]];
    if (q < 0) continue;
    ls.kept_of_local[q] = (int)k;
    ls.kept_pt.push_back(q); ls.kept_cam.push_back(3 * (*in.retained_cam)[k] + (int)(k % 3));
    ls.kept_home.push_back(q < ls.P_own ? 1 : 0); ls.kept_global.push_back((int)k);
  }
  for (size_t k = 0; k < ls.kept_pt.size(); ++k)
    for (int o = pt_start[ls.kept_pt[k]]; o < pt_start[ls.kept_pt[k] + 1]; ++o) { ls.kept_obs.push_back(o); ls.kept_obs_slot.push_back((int)k); }
  return ls;
}

// pair lists: for every point that is eliminated, every (larger camera, smaller camera) pair of its observations
void add_pair_lists(LocalStructure* ls, int C, int long_segment) {
  const std::vector<int>&pt_start = ls->pt_start, &cam = ls->cam, &pt = ls->pt, &kept_of_local = ls->kept_of_local;
  const int P = ls->P, N = ls->N;
  std::vector<int>&dup_a = ls->dup_a, &dup_b = ls->dup_b, &dup_cam = ls->dup_cam;  // (observation indices here; record slots below)
  std::vector<int>&pair_row = ls->pair_row, &pair_col = ls->pair_col, &seg_start = ls->seg_start, &seg_row = ls->seg_row, &seg_col = ls->seg_col;
  // Two residual blocks on one (camera, point) pair (the reference's set-up loop adds whatever the file holds: EX/SimpleBundleAdjuster.scala:139-145):
  // both observations enter every sum; their cross term of the Schur complement belongs to the camera's diagonal block (BalDev::dup_*)
  bool has_dup = false;
  for (int o = 1; o < N && !has_dup; ++o) has_dup = pt[o] == pt[o - 1] && cam[o] == cam[o - 1];
  size_t npairs = 0;
  for (int q = 0; q < P; ++q) { if (kept_of_local[q] >= 0) continue; const size_t k = pt_start[q + 1] - pt_start[q]; npairs += k * (k - 1) / 2; }
  if (has_dup) {
    npairs = 0;
    for (int q = 0; q < P; ++q) {
      bool q_dup = false;
      for (int b = pt_start[q] + 1; b < pt_start[q + 1]; ++b)
        for (int a = pt_start[q]; a < b; ++a) {
          if (cam[b] != cam[a]) { if (kept_of_local[q] < 0) ++npairs; continue; }
          q_dup = true;
          dup_a.push_back(a); dup_b.push_back(b); dup_cam.push_back(cam[a]);
        }
      if (q_dup && kept_of_local[q] >= 0) { ls->error = "internal: a retained point has two residual blocks on one camera"; return; }
    }
    // camera by camera (bal_dup_diag_kernel: one workgroup per camera's run)
    std::vector<int> ord(dup_cam.size());
    std::iota(ord.begin(), ord.end(), 0);
    std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return dup_cam[x] < dup_cam[y]; });
    std::vector<int> a2(ord.size()), b2(ord.size()), c2(ord.size());
    for (size_t k = 0; k < ord.size(); ++k) { a2[k] = dup_a[ord[k]]; b2[k] = dup_b[ord[k]]; c2[k] = dup_cam[ord[k]]; }
    dup_a.swap(a2); dup_b.swap(b2); dup_cam.swap(c2);
  }
  if (npairs > 2000000000ull) { ls->error = "pair list too large"; return; }
  pair_row.resize(npairs); pair_col.resize(npairs);
  {
    const size_t CC = (size_t)C * C;
    std::vector<unsigned> count(CC + 1, 0);  // key = row * C + col
    for (int q = 0; q < P; ++q) {
      if (kept_of_local[q] >= 0) continue;
      for (int b = pt_start[q] + 1; b < pt_start[q + 1]; ++b)
        for (int a = pt_start[q]; a < b; ++a) if (cam[b] != cam[a]) count[(size_t)cam[b] * C + cam[a] + 1]++;
    }
    seg_start.push_back(0);
    std::vector<unsigned> pos(CC, 0);
    unsigned run = 0;
    for (size_t key = 0; key < CC; ++key) {
      pos[key] = run;
      if (count[key + 1]) { seg_row.push_back((int)(key / C)); seg_col.push_back((int)(key % C)); run += count[key + 1]; seg_start.push_back((int)run); }
    }
    for (int q = 0; q < P; ++q) {  // ascending point => entries of a segment are in ascending point order
      if (kept_of_local[q] >= 0) continue;
      for (int b = pt_start[q] + 1; b < pt_start[q + 1]; ++b)
        for (int a = pt_start[q]; a < b; ++a) { if (cam[b] == cam[a]) continue; const unsigned e = pos[(size_t)cam[b] * C + cam[a]]++; pair_row[e] = b; pair_col[e] = a; }
    }
  }
  // the pair lists address the What records, which are in camera-major order (bal_kernels.hpp: kWs)
  for (std::vector<int>* v : {&pair_row, &pair_col, &dup_a, &dup_b}) for (int& x : *v) x = ls->slot[x];
  // Both lists stay in (row camera, column camera) order: neighbouring waves then gather the records of the same
  // points.  (Round 1 sorted the long list by length, longest first, against a long tail: 2.14 ms on Venice-1778 where
  // camera order takes 1.65.  Sorting the short list by length, so that the seven lane groups of a wave finish together,
  // changes nothing in time and fetches 588 MB instead of 345 on Ladybug-1723.)
  // (Round 4 also tried sorting the short list by length inside windows of 224 consecutive segments — the 32 waves that run on
  // one XCD together — so that the seven lane groups of a wave carry segments of like length: bal_pair 131 -> 178 us on
  // Ladybug-1723, 250 -> 322 on Venice-1778.  A wave of seven LONG short segments gathers seven times the records at once;
  // mixed lengths spread that load.  And bal_pair_long at six waves per SIMD (79 VGPRs, no scratch) instead of five: 83-88 ->
  // 87 us, Venice 1088 -> 1130.  Neither kept.)
  // (Round 4 tried the lists in Z-order of (row camera, column camera) — runs of consecutive segments inside small squares of
  // camera pairs, so that the rows' AND the columns' records stay in an XCD's L2: no gain, Schur assembly 0.41 -> 0.42-0.44 ms on
  // Ladybug-1723, 2.46 -> 2.40-2.54 on Venice-1778 for cells of 1, 4 and 16 cameras: the gathers are not bound by L2 misses.)
  for (int g = 0; g < (int)seg_row.size(); ++g) (seg_start[g + 1] - seg_start[g] >= long_segment ? ls->long_segs : ls->short_segs).push_back(g);
}

// ---- the fronts of the reduced camera system ----
FrontLayout layout_fronts(const FrontInputs& in) {
  FrontLayout out;
  FrontHost* fr = out.fr;
  const int C = in.C, cam_b = in.cam_b;
  if (!in.dissected) {
    FrontHost& r = fr[2];
    r.nblk = r.ncols = in.npad / 128; r.cams = C; r.dim = (size_t)in.npad; r.rhs_row = in.rhs_row; r.last = *in.env_last; r.tail = *in.env_tail;
    out.border_blocks = 0;
  } else {
    const std::vector<int>&seg_off = *in.seg_off, &sep_first = *in.sep_first;
    const int nsep = C - cam_b;
    // the leaf fronts this device holds: one device — the head (0) and the tail (1); a rank of a segmented world — its segment (0)
    for (int f = 0; f < 2; ++f) {
      if (in.segmented && f != 0) continue;
      const int seg = in.segmented ? in.role : f;
      const int lo = seg_off[seg], hi = seg_off[seg + 1];
      // the separators next to the segment (cameras of the final numbering): left [ll, lh), right [rl, rh)
      // (the members of a border — pseudo-cameras of retained points, loop-closure cameras — come behind the last separator and are
      // rows of EVERY leaf front: the end of its border, before the right-hand side)
      const int nbm = in.border_members, mf = C - nbm;
      const int ll = seg > 0 ? sep_first[seg - 1] : 0, lh = seg > 0 ? std::min(sep_first[seg], mf) : 0;
      const int rl = seg + 1 < in.segments ? sep_first[seg] : 0, rh = seg + 1 < in.segments ? std::min(sep_first[seg + 1], mf) : 0;
      // first segment: [right | members | rhs]; last: [left reversed | members | rhs]; between two: [right, padded | left | members | rhs] —
      // there the members are tail rows like the left separator's (active in every column)
      const SegmentLayout lay = seg == 0 ? segment_layout(9 * (hi - lo), 0, 9 * (rh - rl + nbm)) : segment_layout(9 * (hi - lo), 9 * (lh - ll + nbm), 9 * (rh - rl));
      FrontHost& L = fr[f];
      L.cams = hi - lo; L.ncols = lay.ncols; L.nblk = lay.nblk; L.dim = (size_t)L.nblk * 128; L.rhs_row = lay.rhs_row; L.tail_rows = lay.tail_rows;
      // rows of every camera in this front: its own interior, or (a separator next to it) the border
      std::vector<int> pos(C, -1);
      std::vector<char> interior(C, 0);
      for (int c = lo; c < hi; ++c) { pos[c] = 9 * (c - lo); interior[c] = 1; }
      const int bo = L.ncols * 128;
      for (int c = rl; c < rh; ++c) pos[c] = bo + lay.right_off + 9 * (c - rl);
      // (the members of a border — one device: the end of the one separator — stay at the END of a reversed border too: their rows are
      // tail rows of the front's envelope, a suffix of the matrix)
      for (int c = ll; c < lh; ++c) pos[c] = bo + lay.left_off + (lay.reversed ? 9 * (lh - 1 - c) : 9 * (c - ll));
      for (int c = mf; c < C; ++c) pos[c] = (seg == 0 ? bo + lay.right_off + 9 * (rh - rl) : bo + lay.left_off + 9 * (lh - ll)) + 9 * (c - mf);
      if (nbm > 0 && !lay.spike) L.last = front_envelope(*in.ocam, *in.opt, pos, interior, in.P, L.nblk, L.tail_rows, pos[mf], &L.tail);
      else L.last = front_envelope(*in.ocam, *in.opt, pos, interior, in.P, L.nblk, L.tail_rows);
      out.border_row_h[f].assign(std::max(1, nsep), 0);
      for (int c = cam_b; c < C; ++c) out.border_row_h[f][c - cam_b] = pos[c] >= 0 ? pos[c] : 0;  // (a separator that is not next to the segment: no block of it here)
      if (in.segmented) {
        // border index -> root index (cholesky_border_add, cholesky_gather_map): separator cameras, and the right-hand-side row
        out.leaf_map_h.assign((size_t)(L.nblk - L.ncols) * 128, -1);
        for (int c = cam_b; c < C; ++c) if (pos[c] >= 0) for (int k = 0; k < 9; ++k) out.leaf_map_h[pos[c] - bo + k] = 9 * (c - cam_b) + k;
        out.leaf_gmap_h = out.leaf_map_h;
        out.leaf_map_h[L.rhs_row - bo] = 9 * nsep;
      }
    }
    out.border_blocks = in.segmented ? fr[0].nblk - fr[0].ncols : (9 * nsep + 1 + 127) / 128;
    FrontHost& r = fr[2];
    r.nblk = r.ncols = (9 * nsep + 1 + 127) / 128; r.cams = nsep; r.dim = (size_t)r.nblk * 128; r.rhs_row = 9 * nsep;
    r.last = *in.root_last;  // (one separator: dense)
    r.tail = *in.root_tail;
    if (!in.segmented) {
      // one device: the tail's border in the root's order — camera order reversed, coordinates in order (pseudo-cameras: in place)
      out.mapB.assign((size_t)out.border_blocks * 128, -1);
      const int nreal = nsep - in.border_members;
      for (int k = 0; k < nsep; ++k) for (int c = 0; c < 9; ++c) out.mapB[9 * k + c] = k < nreal ? 9 * (nreal - 1 - k) + c : 9 * k + c;
      out.mapB[9 * nsep] = 9 * nsep;  // right-hand-side row
      out.mapB_involution = true;  // (a reversal of the real separator cameras, the rest in place)
      for (size_t i = 0; i < out.mapB.size() && out.mapB_involution; ++i) if (out.mapB[i] >= 0 && out.mapB[(size_t)out.mapB[i]] != (int)i) out.mapB_involution = false;
    }
  }
  size_t s_off = 0, linv_off = 0, y_off = 0;  // each front is a dense dim x dim matrix inside one buffer
  for (int f = 0; f < 3; ++f) {
    fr[f].s_off = s_off; fr[f].linv_off = linv_off; fr[f].y_off = y_off;
    s_off += fr[f].dim * fr[f].dim; linv_off += (size_t)fr[f].ncols * 128 * 128; y_off += fr[f].dim;
  }
  return out;
}


// The segmented distribution's plan as the solver derives it (BalSolver::setup), from host data alone: for every residual
// block the segment its camera belongs to (0 .. segments - 1; -k for a camera of separator k, 1 <= k < segments) and the rank
// that owns its point.  Returns the number of segments (1: the sequence was not cut).  Rank-invariant by construction: the
// same code every rank runs.
int bal_segment_plan(const Problem& p, int max_segments, bool forced, std::vector<int>* block_camera_part, std::vector<int>* block_point_owner) {
  std::vector<int> cam_block, pt_block, ocam, opt;
  bal_index_problem(p, &cam_block, &pt_block, &ocam, &opt);
  const int C = (int)cam_block.size(), P = (int)pt_block.size();
  // the order without border or retained points, with the memory order (as the ranks do when their address orders agree); then the
  // cut of a world of max_segments ranks
  const ReducedSystemPlan rp = plan_reduced_system(p, cam_block, ocam, opt, C, P, true, false, SK_BORDER_OFF, SK_RETAINED_OFF, 0);
  for (int& c : ocam) c = rp.order.id[c];
  const std::vector<int> none;
  const BandStructure band{&ocam, &opt, C, P, &none, &none, &none, &none, 0, &rp.order.last, &none, (9 * C + 1 + 127) / 128, 0, 0};
  const CutFlags flags{true, false, false, false, SK_DISSECTION_AUTO, forced ? SK_DISTRIBUTION_SEGMENTED : SK_DISTRIBUTION_AUTO, max_segments, max_segments, -1};
  CutModel model;
  const CutPlan sg = plan_cuts(band, flags, &model);
  const int R = (int)sg.a.size() + 1;
  std::vector<int> part(C, 0);  // per camera of the banded numbering
  for (int c = 0; c < C; ++c) {
    int seg = 0;
    for (int k = 0; k < R - 1; ++k) {
      if (c >= sg.a[k] && c < sg.b[k]) { seg = -(k + 1); break; }
      if (c >= sg.b[k]) seg = k + 1;
    }
    part[c] = seg;
  }
  std::vector<int> seg_of_pt(P, -1);
  for (size_t b = 0; b < ocam.size(); ++b) if (part[ocam[b]] >= 0) seg_of_pt[opt[b]] = part[ocam[b]];
  block_camera_part->resize(ocam.size()); block_point_owner->resize(ocam.size());
  for (size_t b = 0; b < ocam.size(); ++b) {
    (*block_camera_part)[b] = part[ocam[b]];
    (*block_point_owner)[b] = seg_of_pt[opt[b]] >= 0 ? seg_of_pt[opt[b]] : opt[b] % R;
  }
  return R;
}

// The camera order and the border of loop-closure cameras as BalSolver::setup derives them (one process), from host data alone.
// final_index_of_block[b]: the position of residual block b's camera inside the reduced system; returns the number of border cameras.
int bal_border_plan(const Problem& p, int mode, std::vector<int>* final_index_of_block, int* gap, double* model_us, double* plain_us, double* fill) {
  std::vector<int> cam_block, pt_block, ocam, opt;
  bal_index_problem(p, &cam_block, &pt_block, &ocam, &opt);
  const int C = (int)cam_block.size(), P = (int)pt_block.size();
  const int npad = ((9 * C + 1 + 127) / 128) * 128, nblk = npad / 128;
  const CameraOrderPlan plan = plan_reduced_system(p, cam_block, ocam, opt, C, P, true, mode != SK_BORDER_OFF, mode, SK_RETAINED_OFF, 0).order;
  final_index_of_block->resize(ocam.size());
  for (size_t b = 0; b < ocam.size(); ++b) (*final_index_of_block)[b] = plan.id[ocam[b]];
  if (gap) *gap = plan.bordered ? plan.border.gap : 0;
  if (model_us) *model_us = plan.bordered ? plan.border.model_us : plan.border.plain_us;
  if (plain_us) *plain_us = plan.border.plain_us;
  if (fill) {
    *fill = BlockEnvelope(nblk, plan.last.data(), plan.tail.empty() ? nullptr : plan.tail.data()).blocks() / (0.5 * nblk * (nblk + 1.0));
  }
  return plan.bordered ? plan.border.border_cams : 0;
}

int bal_retained_plan(const Problem& p, int mode, int max_points, int border_mode, std::vector<int>* retained_of_block, double* model_us, double* model_us_without, bool with_memory_order) {
  std::vector<int> cam_block, pt_block, ocam, opt;
  bal_index_problem(p, &cam_block, &pt_block, &ocam, &opt);
  const int C = (int)cam_block.size(), P = (int)pt_block.size();
  const ReducedSystemPlan rp = plan_reduced_system(p, cam_block, ocam, opt, C, P, with_memory_order, border_mode != SK_BORDER_OFF, border_mode, mode, max_points);
  std::vector<char> kept(P, 0);
  for (int q : rp.retained) kept[q] = 1;
  retained_of_block->resize(ocam.size());
  for (size_t b = 0; b < ocam.size(); ++b) (*retained_of_block)[b] = kept[opt[b]];
  if (model_us) *model_us = rp.order.model_us;
  if (model_us_without) *model_us_without = rp.without_us;
  return (int)rp.retained.size();
}

}  // namespace sk
