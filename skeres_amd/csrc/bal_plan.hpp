// Host planning of the DENSE_SCHUR path (bal_plan.cpp): everything BalSolver::setup decides from host data alone — the order
// of the cameras inside the reduced system, its border and retained points, where the camera sequence is cut, this rank's
// observations and pair lists, the layout of the fronts.  Pure functions over plain inputs: no device, no collective.
#pragma once
#include <string>
#include <vector>

#include "chol_envelope.hpp"
#include "dev_knobs.hpp"
#include "problem.hpp"

namespace sk {

bool bal_block_shape(const Problem& p, int* r, int* c, int* q);
bool problem_is_bal_shaped(const Problem& p, std::string* why_not);
void bal_index_problem(const Problem& p, std::vector<int>* cam_block, std::vector<int>* pt_block, std::vector<int>* ocam,
                       std::vector<int>* opt);
void bal_partition_points(const std::vector<int>& opt, int num_points, int world, std::vector<int>* cut);
// the plans as BalSolver::setup derives them (one process), for tests and tools: sk_problem_*_plan
int bal_segment_plan(const Problem& p, int max_segments, bool forced, std::vector<int>* block_camera_part, std::vector<int>* block_point_owner);
int bal_border_plan(const Problem& p, int mode, std::vector<int>* final_index_of_block, int* gap, double* model_us, double* plain_us, double* fill);
// the retained points as BalSolver::setup chooses them (one process): flag per residual block; returns their number
int bal_retained_plan(const Problem& p, int mode, int max_points, int border_mode, std::vector<int>* retained_of_block, double* model_us, double* model_us_without,
                      bool with_memory_order = true);

// The chain model (bal_plan.cpp, namespace chain_model): what the planner's decisions are held against.
namespace chain_model {
// seconds per iteration on one MI355X of the phases that shard with the points, from the problem's pair entries and observations
double shardable_work_s(double pairs, double observations);
double allreduce_triangle_us(double block_rows, int world);  // the bandwidth term of all-reducing a lower triangle of block_rows 128-block rows
double pair_entries(const std::vector<int>& opt, int num_points);  // sum over the points of k (k - 1) / 2, k = the point's observations
}  // namespace chain_model

// ---- the layout of the reduced system (plan_reduced_system) ----
// A camera graph: per observation its camera and its point (see bal_plan.cpp, choose_border).
struct CamGraph { const std::vector<int>* ocam; const std::vector<int>* opt; int C, P; };
struct BorderChoice {
  std::vector<int> new_id;        // banded numbering -> final numbering (band cameras in order, then the border)
  std::vector<int> last, tail;    // bordered envelope (cholesky_envelope_bordered)
  int border_cams = 0, gap = 0, variant = 0;
  double model_us = 0.0, plain_us = 0.0;
};
struct CameraOrderPlan {
  std::vector<int> id;           // first-appearance numbering -> final numbering (pseudo-cameras of retained points: indices >= the real cameras')
  std::vector<int> plain_id;     // ... of the best candidate as it stands (real cameras only; what the retained points are chosen on)
  std::vector<std::vector<int>> candidates;  // the candidate orders this plan was chosen from (camera_order_candidates of g)
  std::vector<int> last, tail;   // the envelope of the reduced system in that numbering (tail: empty unless bordered)
  int candidate = 0;             // 0 first appearance, 1 memory order, 2 RCM
  bool bordered = false;
  BorderChoice border;
  double flops = 0.0;            // trailing-update flops of the envelope
  double model_us = 0.0;         // the chain model of the plan
};
// the two graphs of a problem whose points `points` (slot s -> pseudo-camera C + s / 3) are retained
struct RetainedGraphs {
  std::vector<int> ocam_g, opt_g, ocam_x, opt_x;
  int Cx = 0, Px = 0;
  CamGraph g(int C, int P) const { return CamGraph{&ocam_g, &opt_g, C, P}; }
  CamGraph x() const { return CamGraph{&ocam_x, &opt_x, Cx, Px}; }
};
struct ReducedSystemPlan {
  CameraOrderPlan order;            // over the real cameras and the pseudo-cameras
  std::vector<int> retained;        // the retained points (three to a pseudo-camera, in pseudo-camera order); empty: every point is eliminated
  RetainedGraphs graphs;            // ... and the structure with them (first-appearance numbering)
  double without_us = 0.0;          // the chain model of the plan with every point eliminated
};
ReducedSystemPlan plan_reduced_system(const Problem& p, const std::vector<int>& cam_block, const std::vector<int>& ocam, const std::vector<int>& opt, int C, int P,
                                      bool with_memory_order, bool border_ok, int border_mode, int retained_mode, int retained_max);

// ---- where the camera sequence is cut (plan_cuts) ----
// The reduced system's structure in the banded numbering, as the cut is planned on it.
struct BandStructure {
  const std::vector<int>* ocam; const std::vector<int>* opt;  // every observation: camera (C of them, pseudo-cameras included), point (P)
  int C, P;
  const std::vector<int>* band_ocam; const std::vector<int>* band_opt;  // retained points: the eliminated points' observations over the real cameras
  const std::vector<int>* struct_ocam; const std::vector<int>* struct_opt; int struct_P;  // ... and the structure with pseudo-cameras (empty: ocam / opt)
  const std::vector<int>* env; const std::vector<int>* env_tail;  // the envelope of the chosen order; its tail profile (empty: not bordered)
  int nblk;
  int pseudo_cams, border_members;
};
// no block column of the bordered band is SYRK-bound (the chain model's limit): such a band is dissected in front of its border
bool band_is_chain_bound(const BandStructure& s);
struct CutFlags {
  bool multi, two_seg_try, lockstep_cut, pseudo_border;
  int dissection, distribution_mode, max_segments, world, dissect_at;  // Options::dissection, ::distribution_mode, ::max_segments, ::world; DevKnobs::dissect_at
};
// the chain model's figures behind the cut (sk_solver_stat): kept from pass to pass of setup()'s cut loop
struct CutModel {
  double model_us[9] = {0};   // the prediction per number of segments (index: segments; [1] = undissected)
  double t_plain = 0.0, t_model = 0.0, two_segments_members_us = 0.0;
};
struct CutPlan {
  std::vector<int> a, b;      // the separators [a, b) in the banded numbering, ascending
  // the cut is the lock-step one of a single device: its caller claims the right to two resident servers (a CholeskyContext call) and,
  // when it gets none, drops the cut — unless drop_without_claim is false (a developer's SK_DISSECT_AT stands either way)
  bool needs_pair_claim = false, drop_without_claim = false;
};
CutPlan plan_cuts(const BandStructure& s, const CutFlags& f, CutModel* model);
// The final numbering of a cut sequence: the segments one after the other — the last one REVERSED (it is eliminated back to front) —
// then the separators in sequence order, then the border's members (cameras [Cband, C)).
struct CutNumbering {
  std::vector<int> seg_off;    // first camera of every segment in the final numbering, then the first separator camera
  std::vector<int> sep_first;  // ... and of every separator, then C
  std::vector<int> fin;        // banded numbering -> final numbering
};
CutNumbering apply_cuts(const CutPlan& cuts, int Cband, int C);

// ---- this rank's observations (index_local_structure, add_pair_lists) ----
struct LocalInputs {
  const std::vector<int>* ocam; const std::vector<int>* opt;  // final numbering
  int C, P;
  int world, rank;
  bool segmented; int segments, role; const std::vector<int>* seg_off;
  const std::vector<int>* retained_pts; const std::vector<int>* retained_cam;
};
struct LocalStructure {
  std::string error;                       // not empty: the structure cannot be indexed (SK_ERR_UNSUPPORTED)
  std::vector<int> local_pt; int P_own = 0;  // global point of every local point; the first P_own are this rank's own
  int P = 0, N = 0;                        // local points, local observations
  std::vector<int> pt_start, order, cam, pt;  // point-major, ascending camera within a point; order: residual block of local observation
  const Tape* tape = nullptr;              // the recorded functor of the problem's device-evaluated blocks, if any
  std::vector<double> obs;                 // captured doubles per observation, plane by plane
  std::vector<int> host_obs; std::vector<const CostFunction*> host_cf;  // host-evaluated observations and their cost functions
  std::vector<int> cam_start, cam_obs, slot;  // camera CSR; slot: observation -> place in camera-major order
  std::vector<int> kept_pt, kept_cam, kept_home, kept_global, kept_obs, kept_obs_slot;  // this rank's retained points (BalDev::kept_*)
  std::vector<int> kept_of_local;
  std::vector<int> dup_a, dup_b, dup_cam;  // two residual blocks on one (camera, point) pair: BalDev::dup_*
  std::vector<int> pair_row, pair_col, seg_start, seg_row, seg_col, short_segs, long_segs;
};
LocalStructure index_local_structure(const Problem& p, const LocalInputs& in);
// the pair lists of the eliminated points, in record slots; long_segment: entries from which a camera pair goes to the long list
void add_pair_lists(LocalStructure* ls, int C, int long_segment);

// ---- the fronts of the reduced camera system (layout_fronts) ----
// One front (BalDev::front): 0 head, 1 tail, 2 root.  Not dissected: only the root, which is then the whole system.
struct FrontHost {
  int nblk = 0, ncols = 0, cams = 0;   // block rows; block columns factored here; cameras eliminated here
  size_t dim = 0, s_off = 0, linv_off = 0, y_off = 0;
  int rhs_row = 0;
  int tail_rows = 1;                   // block rows at the end that every column reaches (cholesky_plan): > 1 for a segment between two separators
  std::vector<int> last;               // block envelope (empty: dense)
  std::vector<int> tail;               // tail profile of a bordered envelope (cholesky_factor; empty: the uniform tail_rows)
  const int* env() const { return last.empty() ? nullptr : last.data(); }
  const int* tl() const { return tail.empty() ? nullptr : tail.data(); }
  BlockEnvelope envelope() const { return BlockEnvelope(nblk, env(), tl(), ncols, tail_rows); }
};
struct FrontInputs {
  const std::vector<int>* ocam; const std::vector<int>* opt; int P;  // the reduced system's structure (with pseudo-cameras), final numbering
  int C, npad, rhs_row;
  const std::vector<int>* env_last; const std::vector<int>* env_tail;    // undissected: the root is the whole system
  bool dissected, segmented; int segments, role;
  const std::vector<int>* seg_off; const std::vector<int>* sep_first; int cam_b, border_members;
  const std::vector<int>* root_last; const std::vector<int>* root_tail;
};
struct FrontLayout {
  FrontHost fr[3];
  std::vector<int> border_row_h[2];   // separator camera -> row of a leaf's border
  std::vector<int> leaf_map_h, leaf_gmap_h;  // segmented: border index -> root index (gmap: rhs row -> -1)
  std::vector<int> mapB;              // one device, dissected: the tail's border index -> root index
  bool mapB_involution = false;
  int border_blocks = 0;
};
FrontLayout layout_fronts(const FrontInputs& in);

}  // namespace sk
