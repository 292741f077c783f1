// ba_kernels.h -- launch interface of the BA device kernels (internal).
#pragma once
#include <algorithm>
#include <vector>
#include <hip/hip_runtime.h>
#include <cstdint>

#include "dense_cholesky.h"
#include "ba_fused_slices.h"

namespace thip {

// One workgroup of the fused linearise + Schur kernel (ba_fused.hip): consecutive wave tiles whose tracks see at
// most kFusedMaxCams variable cameras.  Sub-chunks of 4 tiles are linearised into LDS; the pair products
// What_a What_b^T of every track are accumulated in registers by the lane that owns the target block (la, lb).
struct FusedRun {
  int tile0, ntiles;     // wave tiles of the run
  int cam_off, W;        // local camera table: frun_cams[cam_off + lc] = reduced camera index (ascending)
  int tgt_off, ntgt;     // target blocks: frun_tgt[tgt_off + k] = la | lb << 8 (lb <= la)
  int part_off;          // doubles offset of the run's partial sums: [ntgt][36] then [W][6][3]
  int gp;                // G | PS << 8.  G = consumer waves per track slice: 1, 2 or 4 (64 G >= max(ntgt, 6 W));
                         // PS = track slices per consumer wave (only with G == 1): floor(64 / PS) >= ntgt, 6 W <= 64
                         // | kFusedUnequalSlices (ba_fused_slices.h; k_lin_schur, G == 1): the PS slices are listed behind the run's
                         // targets, frun_tgt[tgt_off + ntgt + g] = lane offset | width << 8 -- slice g owns the first `width` targets
  int stage_off, nstage; // ba_fused.hip: frun_stage[stage_off + k] = camera index of the k-th per-camera block the run keeps in
                         // LDS: its W local cameras, then the CONSTANT cameras its tracks see (obs_lc = 0x80 | index among them)
};
inline int fused_tiles_per_subchunk(int) { return 4; }   // one wave per tile, 256-thread workgroups
constexpr int kFusedMaxCams = 22;        // -> at most 253 target blocks = one per thread
constexpr int kFusedMaxConst = 22;       // constant cameras a run may see (their blocks are staged in LDS next to the local cameras')
constexpr int kFusedMaxStage = kFusedMaxCams + kFusedMaxConst;
constexpr int kFusedTileTracks = 32;     // tracks per wave tile (128 per sub-chunk)
// fused assembly with intrinsics (ba_fused_intr.hip): compound camera blocks [extrinsics (6) | compact intrinsics rows (4)]
constexpr int kFusedIntrRows = 4, kFusedIntrWidth = 6 + kFusedIntrRows;
constexpr int kFusedMaxCamsIntr = 12;    // -> at most 78 target blocks x 3 lanes
constexpr int kFusedMaxConstIntr = 12;   // constant cameras a run of the compound-block plan may see (staged in LDS as above)
constexpr int kFusedMaxStageIntr = kFusedMaxCamsIntr + kFusedMaxConstIntr;

// Device-resident problem (SoA, observations sorted by point and packed into
// wave tiles of <= 64 observations that never split a point).
struct DevProblem {
  int nc, np, ncv, ntiles;
  int64_t nobs;
  int n;                       // reduced system size = 6 * ncv
  int pd;                      // point tangent dofs: 3 (SphereManifold<4>) or 4
  int loss_type;
  double loss_width;
  const double* intr;          // [ng][10]
  const int* group_model;      // [ng]
  const int* cam_group;        // [nc]
  const int* cam_red;          // [nc] reduced index or -1
  const uint8_t* cam_mask;     // [nc] bit q = extrinsics column q frozen
  const uint8_t* pt_const;     // [np]
  const double2* obs_uv;       // [nobs]
  const double2* obs_si;       // [nobs] or nullptr
  const int* obs_cam;          // [nobs]
  const int* obs_pt;           // [nobs]
  const int* tile_start;       // [ntiles]
  const int* tile_count;       // [ntiles]
  // tracks with > 64 observations (slow path, ba_kernels.hip "long tracks")
  int long_nobs, long_ntracks;
  const int* long_obs_index;   // [long_nobs] index into the sorted observation arrays
  const int* long_obs_slot;    // [long_nobs]
  const int* long_track_start; // [long_ntracks + 1]
  const int* long_track_pt;    // [long_ntracks]
  const double* scale_c;       // [nc][6] Jacobi scaling
  const double* scale_p;       // [np][pd]
  // intrinsics blocks (intrinsics_to_optimize != NONE): they come FIRST in the
  // reduced system, 10 slots per variable group; cameras follow at ni + 6 * rc
  int ni;                      // 10 * (#variable intrinsics groups), 0 = all intrinsics constant
  int ng_total;                // number of intrinsics groups
  const int* grp_k;            // [ng] number of parameters K of the group's model
  const int* grp_red;          // [ng] reduced group index or -1
  const unsigned* grp_free;    // [ng] bit q = parameter q is free
  const unsigned* red_free;    // [#variable groups] the same mask by reduced group index
  int intr_rows;               // intrinsics rows stored per record: 10, or 4 compact rows (k-th free parameter)
  const double* scale_i;       // [ng][10] Jacobi scaling of the intrinsics columns
  const double* intr_cand;     // [ng][10] candidate intrinsics (back-substitution / trial cost)
  const double* scale_red;     // [n] Jacobi scaling by reduced index (finalize)
  // gather-based Schur assembly (k_lin_obs + k_schur_diag + k_schur_blocks), ni == 0:
  // static lists built at create()
  double* rec;                 // per-observation records, camera-major: [#records][6*pd + 14] = {What | F | r} without
                               // intrinsics (What = W Li^T with V^-1 = Li^T Li; gp holds ghat = Li g of slot_pt),
                               // [#records][12*pd + 20 + 2*KI*pd + 3*KI] with intrinsics, KI = intr_rows (ba_kernels.hip)
  const uint8_t* obs_kind;     // [nobs] (sorted order) THEIA_OBS_* or null: depth-prior rows use the pseudo model
  double loss_width_depth;     // robust_loss_width_depth_prior
  const int* slot_pt;          // [#records] point of a record slot (records without intrinsics)
  const int* rec_slot;         // [nobs_main] record slot of a (sorted) observation, -1 = none
  const int* slot_obs;         // [#records] inverse: (sorted) observation of a record slot
  int n_diag_items, n_blk_items;
  const int* diag_items;       // [n_diag_items][4] {rc, first slot, end slot, atomic}
  const int* blk_items;        // [n_blk_items][5] {ri, rj, beg, end, atomic}
  const int2* blk_pairs;       // (slot of the obs of camera ri, slot of the obs of camera rj) of a common track
  const int* pt_sum_slot;      // [np] or null: pseudo-record slot of a track's summed intrinsics fields (k_lin_obs_intr), -1 = none
  const uint8_t* slot_in_sum;  // [#records] or null: the observation's track is summed (its own pair term is in the sum)
  const uint8_t* pt_sum_cnt;   // [np]: pseudo-records (summed groups) of a track, pt_sum_slot[p] .. + cnt - 1
  const int* sum_group;        // [#pseudo-records] reduced group of pseudo-record sum_base + j
  int sum_base;
  // fused linearise + Schur (ba_fused.hip), ni == 0: static plan built at create()
  int n_fruns;
  const FusedRun* fruns;
  const int* frun_order;       // [n_fruns] run indices, most expensive first: the order in which workgroups take runs
  int* frun_next;              // [2] work-queue heads of k_lin_schur / k_backsub_runs (zeroed by k_cam_prep before every launch)
  const int* frun_cams;
  const int* frun_stage;       // camera indices of the per-camera blocks a run stages in LDS (FusedRun::stage_off / nstage)
  const unsigned short* frun_tgt;
  const uint8_t* obs_lc;       // [nobs_main] local camera index inside the run; constant camera: 0x80 | index among the run's
                               // constant cameras (staged in LDS behind the W local ones: slot W + (lc & 0x7f)), for every
                               // block width (ba_fused.hip, ba_fused_intr.hip); tracks outside the runs keep 0xFF
  const uint8_t* obs_tl;       // [nobs_main] track index inside the sub-chunk
  const int* tile_trk_end;     // [ntiles] tracks of the sub-chunk up to and including this tile
  double* fpart;               // per-run partial sums
  double* camrot;              // [nc][kCamRot] per-camera blocks at the linearisation point (k_cam_prep), null = not in use
  double* camrot_cand;         // the same for the candidate cameras of the trial step (back-substitution)
  double* camdir;              // [nc][12] the trial step of each camera as {D (3 x 3), v (3)} (camera_step_direction; k_cam_update)
  int camrot_current;          // host-set per launch: camrot already holds the blocks of `cam` (launch_linearize_fused skips k_cam_prep)
  // The folded LM chain (ba_solver.hip: lm_glue_applies): which of the two parameter buffers holds the state is a number on
  // the device, LmState::cur, flipped by the control kernel on an accepted step instead of a copy.  lm_cur != null (host-set
  // for the bodies of such a run): k_lin_schur, k_cam_update<1> and k_backsub_runs read it once per workgroup and, where it is
  // 1, take camrot / camrot_cand and their state / candidate arguments the other way round (lm_flip); pts_alt: the point
  // buffer k_lin_schur linearises at then.  Null everywhere else: the buffers are the ones passed.
  const int* lm_cur;
  const double* pts_alt;
  unsigned model_mask;         // bit m = some intrinsics group uses camera model m (picks the kernel instance)
  int fused_dbg;               // development switches (THEIA_HIP_FUSED_DBG): 1 = skip phase S, 2 = skip phase L arithmetic
  int n_sum_items;
  const int* sum_items;        // [n_sum_items][6] {ri, rj, tbeg, tend, dbeg, dend} into sum_src
  const int* sum_src;          // offsets into fpart
  // fused_bw > 0 (ba_fused_intr.hip): the camera-side blocks are fused_bw wide, a local camera of a run is a camera with a
  // variable extrinsics block OR a variable intrinsics group, sum_items / sum_src are the generic lists of k_sum_items
  // (n_sum_items first-level items followed by n_sum_items2 second-level ones; sources are int pairs)
  int fused_bw, n_sum_items2;
  unsigned fused_kmask;        // the free-parameter mask every variable intrinsics group shares, 0 = they differ
  // camera priors in use (compact list): 3 residuals each on one camera's extrinsics
  int n_priors;
  const int* prior_cam;        // [n_priors] camera index
  const int* prior_kind;       // [n_priors] THEIA_PRIOR_* bit
  const double* prior_vec;     // [n_priors][3]
  const double* prior_info;    // [n_priors][9] sqrt information, row-major
};

// Per-iteration reduced-system workspace: one contiguous buffer so that a
// single memset clears it and a single all-reduce sums it across ranks.
//   [ S (n*n) | rhs (n) | colsq (n) | gc (n) | scalars (16) ]
struct ReduceBuf {
  double* base;
  size_t count;     // doubles
  double* S; double* rhs; double* colsq; double* gc; double* scal;
};
enum {  // indices into ReduceBuf::scal: [0,8) are SUM-reduced, [8,16) MAX-reduced
  SC_COST = 0,      // sum 1/2 rho at x
  SC_INVALID = 1,   // > 0 if any functor returned false
  SC_NOTPD = 2,     // > 0 if a point block / the reduced matrix was not PD
  SC_GMAX = 8,      // max |gradient| (points part; cameras folded in by finalize)
  SC_COUNT = 16
};

// Inner iterations (ba_inner.hip): one sweep of block coordinate descent over the parameter buffers cam / pts / intr
// (cameras, then shared intrinsics, then points), each block by its own LM solve.
struct InnerArgs {
  DevProblem P;                 // topology, masks, loss (P.intr is not used: the intrinsics come from `intr`)
  const int* cam_obs_off;       // [nc + 1] per camera: range of cam_obs_idx
  const int* cam_obs_idx;       // (sorted) observation indices of the camera
  const int* grp_obs_off;       // [ng + 1], [..]: the same per intrinsics group (only with variable intrinsics)
  const int* grp_obs_idx;
  const int* trk_off;           // [ntracks + 1] observation ranges of the tracks in the sorted arrays
  int ntracks;
  int64_t nobs;                 // observations that enter the cost (sorted arrays, fixed residual blocks excluded)
  double* cam; double* pts; double* intr;   // in / out
  const int* gate;              // device flag: 0 = return at once
  int has_si = 0, has_kind = 0;  // set by the launchers: P.obs_si / P.obs_kind are real (otherwise valid stand-ins)
  int own_rank = 0, own_world = 1;   // sharded inner iterations: this launch sweeps the cameras / groups with index % own_world == own_rank
  // the intrinsics sweep with grp_wgs > 1 workgroups per group (co-resident: cooperative launch): per group and pass parity
  // grp_wgs partial sums of kInnerGroupSums doubles in grp_part, arrival counters in grp_bar ([ng] counters | abort flag | [ng] done flags | pad, zeroed before the launch)
  double* grp_part = nullptr; int* grp_bar = nullptr; int grp_wgs = 1; int grp_max_polls = 200000;
  int grp_parts = 1;            // parts a pass over a group's observations is dealt to (= the cooperative launch's workgroups per group; the one-workgroup launch walks them in order)
};
constexpr int kInnerGroupSums = 68;        // 55 (J'J, packed) + 10 (J'r) + cost + invalid count (+ 1 pad)
constexpr int kInnerGroupMaxWgs = 32;
inline int inner_group_wgs(int ng_total) { return std::max(1, std::min(kInnerGroupMaxWgs, 256 / std::max(1, ng_total))); }   // <= 256 co-resident workgroups (one per CU at this kernel's register count: 512 were refused)
void launch_inner_sweep(const InnerArgs& A, hipStream_t st, int stages = 7);   // stages: 1 cameras, 2 intrinsics groups, 4 points
// out[0] = |x0 - x|^2, out[1] = |x|^2 over the variable blocks
void launch_inner_norms(const InnerArgs& A, const double* cam0, const double* pts0, const double* intr0, double* out2, double* part,
                        hipStream_t st, int which = 0);   // part: scratch of 2 * kInnerCostBlocks doubles; which: 0 all blocks, 1 points, 2 cameras + intrinsics
// sharded inner iterations: a shard's candidate points into the (zeroed) global point buffer; the sweep's scalars
void launch_inner_scatter_points(int np, const double* pts, const int* global_index, double* gpts, hipStream_t st);
void launch_inner_combine(const double* reduced4, const double* cam2, double* out4, hipStream_t st);
// blocks of `stride` doubles: keep those with index % world == rank, zero the others (the ranks' buffers are then summed)
void launch_inner_keep_owned(double* x, int nblocks, int stride, int rank, int world, hipStream_t st);
// cost of every residual block at (cam, pts, intr): out[0] = sum rho / 2 (+ camera priors), out[1] > 0 if a functor failed;
// part: scratch of 2 * kInnerCostBlocks doubles
constexpr int kInnerCostBlocks = 512;
void launch_inner_cost(const InnerArgs& A, double* part, double* out2, hipStream_t st);
// both in two launches (the unsharded sweep): out4 = {step^2, |x|^2, cost, invalid}; part: 4 * kInnerCostBlocks doubles
void launch_inner_norms_cost(const InnerArgs& A, const double* cam0, const double* pts0, const double* intr0, double* out4, double* part,
                             hipStream_t st);

// Which template instance the launch sites of the fused and the inner-iteration kernels take.  Each launch site branches
// on the value its file's helper returns, and theia_hip_ba_kernel_instances (ba_query.hip) prints the same value: the
// report cannot drift from the dispatch.
struct FusedInstance {   // k_lin_schur, k_backsub_runs (ba_fused.hip), k_lin_schur_i (ba_fused_intr.hip)
  int pd;          // point parametrisation: 3 or 4
  bool trig;       // kModelsAll (an FOV or fisheye group is present), else kModelsNoTrig
  int lossk;       // LOSSK of the instance
  int waves;       // k_backsub_runs: waves per SIMD the register allocation aims at (2 or 3)
  int bw;          // free intrinsics: the compound block width (9, 10, 13, 16), else 0
  bool kmask;      // free intrinsics: the FOCAL_LENGTH | RADIAL_DISTORTION instance
};
FusedInstance lin_schur_instance(const DevProblem& P);          // launch_linearize_fused, launch_linearize_fused_first
FusedInstance lin_schur_intr_instance(const DevProblem& P);     // launch_linearize_fused_intr
bool backsub_runs_applies(const DevProblem& P);                 // launch_backsub_runs takes the step (else: k_backsub)
FusedInstance backsub_runs_instance(const DevProblem& P);
bool backsub_runs_intr_applies(const DevProblem& P);            // the same for launch_backsub_runs_intr
FusedInstance backsub_runs_intr_instance(const DevProblem& P);
struct InnerInstance {   // k_inner_views, k_inner_groups, k_inner_tracks (ba_inner.hip)
  bool lean;       // k_inner_views / k_inner_groups: kModelsNoTrig with loss class lossk1; otherwise <kModelsAll, 2>
  int lossk1;      // 0 trivial, 1 any other loss (only read when lean)
  bool priors;     // k_inner_views: the instance with camera priors
  int kc;          // k_inner_groups: rows per group, 4 or 10
  int pd; bool trig; int lossk;   // k_inner_tracks
};
InnerInstance inner_instance(const DevProblem& P);              // launch_inner_sweep
// which assembly launch_linearize takes for the tracks inside a wave tile
enum LinRoute { LIN_NONE = 0, LIN_FUSED, LIN_FUSED_INTR, LIN_GATHER_INTR, LIN_GATHER };
LinRoute linearize_route(const DevProblem& P);

void launch_colnorm(const DevProblem& P, const double* cam, const double* pts, double* colsq_c,
                    double* colsq_p, double* colsq_i, hipStream_t st);
void launch_build_scale_red(const DevProblem& P, double* scale_red, hipStream_t st);
void launch_make_scale(int count, const double* colsq, double* scale, hipStream_t st);
void launch_linearize(const DevProblem& P, const double* cam, const double* pts, const double* radius /* device */,
                      const ReduceBuf& rb, double* Vinv, double* gp, double* tile_part,
                      hipStream_t st);
// fused path: k_cam_prep + k_lin_schur + k_schur_sum (S blocks are WRITTEN, the buffer must be clear where nothing lands)
// glue (the folded LM chain, ba_solver.hip: lm_glue_applies): k_schur_sum also adds the LM diagonal, folds the camera
// gradient into rb.scal[SC_GMAX], writes the entries k_sp_symm would mirror (symm_map / nt: chol_plan_tile_lists) and, with
// red_out, carries the first stage of the reduction of tile_part's four fields (fmaxflag) -- no k_finalize_rcs, no k_sp_symm
struct LinGlue { const double* scale_red; const int* symm_map; int nt; const int* fmaxflag; double* red_out; };
void launch_linearize_fused(const DevProblem& P, const double* cam, const double* pts, const double* radius /* device */,
                            const ReduceBuf& rb, double* Vinv, double* tile_part, hipStream_t st, const LinGlue* glue = nullptr);
// the first linearisation of a solve with the Jacobi scaling folded in (no separate column-norm pass): P is the solve's view,
// the kernels run on unit scales and leave scale_p, scale_c and scale_red; the reduced system in rb is the UNIT-camera-scale
// one until the caller has rescaled it (chol_plan_rescale with scale_red), and P.camrot holds unit-scale blocks
void launch_linearize_fused_first(const DevProblem& P, const double* ones_c, const double* ones_p, double* scale_c, double* scale_p,
                                  double* scale_red, const double* cam, const double* pts, const double* radius /* device */,
                                  const ReduceBuf& rb, double* Vinv, double* tile_part, hipStream_t st);
void launch_linearize_fused_intr(const DevProblem& P, const double* cam, const double* pts, const double* radius /* device */,
                                 const ReduceBuf& rb, double* Vinv, double* tile_part, hipStream_t st);
// colsq_c[nc][6] / colsq_i[ng][10] += the squared column norms k_sum_items left by reduced index (Jacobi scaling)
void launch_scatter_colsq(const DevProblem& P, const double* colsq_red, double* colsq_c, double* colsq_i, hipStream_t st);
// per-camera blocks (rotation terms, masked scaling, intrinsics) of `cam` -> camrot (ba_fused.hip)
void launch_cam_prep(const DevProblem& P, const double* cam, const double* intr, double* camrot, hipStream_t st, const double* ycam = nullptr);
// K4 + K5 by persistent workgroups over the fused plan's runs (ba_fused.hip: k_backsub_runs); false = not applicable
bool launch_backsub_runs(const DevProblem& P, const double* pts, double* cand_pts, const double* Vinv, double* tile_part, hipStream_t st);
bool launch_backsub_runs_intr(const DevProblem& P, const double* pts, double* cand_pts, const double* Vinv, double* tile_part,
                              const double* y, hipStream_t st);   // the compound-block plan (free intrinsics); y: the solved step
void launch_reduce_tiles(int ntiles, const double* tile_part, int nfields, const int* field_to_scal,
                         const int* field_is_max, double* scal, hipStream_t st, double* red_part = nullptr);
// first stage of a two-stage reduction: kReduceBlocks workgroups fold contiguous slices of the per-tile partials into
// out[kReduceBlocks][nfields] (fixed order); the one-workgroup consumers then reduce kReduceBlocks rows instead of ntiles
constexpr int kReduceBlocks = 128;
void launch_reduce_tiles_stage1(int ntiles, const double* tile_part, int nfields, const int* field_is_max, double* out,
                                hipStream_t st);
// camera priors (ba_priors.h).  mode: PRIOR_COLNORM adds the squared column norms of their (unscaled) Jacobians
// to colsq_c[nc][6]; PRIOR_LINEARIZE adds J'J / J'r / g / column norms / cost to the reduced system at `cam`;
// PRIOR_TRIAL adds the model-cost change of the step y and the cost at `cand_cam` to scal_cost / scal_mcc;
// PRIOR_COST adds the cost at `cam` to *scal_cost; PRIOR_FIXED the cost of the priors of CONSTANT cameras.
enum { PRIOR_COLNORM = 0, PRIOR_LINEARIZE = 1, PRIOR_TRIAL = 2, PRIOR_COST = 3, PRIOR_FIXED = 4 };
void launch_cam_priors(const DevProblem& P, int mode, const double* cam, const double* cand_cam, const double* y,
                       const ReduceBuf* rb, double* colsq_c, double* scal_cost, double* scal_mcc, hipStream_t st);
// tile_part != null: the kernel first folds the per-tile partial sums of the linearisation into rb.scal
// (= launch_reduce_tiles cfg 0), saving that launch; only when no all-reduce sits between the two.
void launch_finalize_rcs(const DevProblem& P, const double* radius /* device */, const ReduceBuf& rb, hipStream_t st,
                         int ntiles = 0, const double* tile_part = nullptr, const int* f2s = nullptr,
                         const int* fmaxflag = nullptr, const uint8_t* tile_cls = nullptr, int want_cls = 0);
int cam_update_preps(const DevProblem& P);   // 1 / 2: launch_cam_update writes the candidate's per-camera blocks itself (1: no free intrinsics)
// glue (the folded LM chain; fused path without intrinsics only): further workgroups of the launch zero the tiles zero_items
// of the reduced system zero_S (chol_plan_tile_lists), which is dead once the solve has left y, and, with lin_part, one folds
// the linearisation's scalars (lin_ntiles rows of 4 fields, k_schur_sum's stage-1 sums or the per-tile partials) into scal
struct CamUpdateGlue {
  double* zero_S; const int* zero_items; int nzero; int prep_blocks;
  const double* lin_part; int lin_ntiles; const int* lin_f2s; const int* lin_fmaxflag; double* scal;
};
void launch_cam_update(const DevProblem& P, const double* cam, const double* y, double* cand_cam,
                       double* cand_intr, double* out_stepsq, double* out_xnormsq, hipStream_t st, double* zero16 = nullptr,
                       const CamUpdateGlue* glue = nullptr);
void launch_backsub(const DevProblem& P, const double* cam, const double* pts, const double* cand_cam,
                    double* cand_pts, const double* yc, const double* Vinv, double* tile_part,
                    double* scal, hipStream_t st);
void launch_evaluate(const DevProblem& P, const double* cam, const double* pts, double* residuals,
                     double* jac_cam, double* jac_pt, uint8_t* valid, double* tile_part,
                     hipStream_t st, double* jac_intr = nullptr);
void launch_cost_only(const DevProblem& P, const double* cam, const double* pts, double* tile_part,
                      double* scal, hipStream_t st);

void launch_long_colnorm(const DevProblem& P, const double* cam, const double* pts, double* colsq_c, double* colsq_p,
                         double* scratch, hipStream_t st, double* colsq_i = nullptr);
void launch_long_linearize(const DevProblem& P, const double* cam, const double* pts, const double* radius /* device */, const ReduceBuf& rb,
                           double* Vinv, double* gp, double* scratch, hipStream_t st);
void launch_long_backsub(const DevProblem& P, const double* cam, const double* pts, const double* cand_cam,
                         double* cand_pts, const double* yc, const double* Vinv, double* scratch, double* scalB,
                         hipStream_t st);

// the dense SPD solve (dense_cholesky.hip): dense_cholesky.h

// Tile-sparse, nested-dissection ordered, level-scheduled variant of the same
// solve (sparse_cholesky.hip).  adj = symmetric nt x nt (nt = ceil(n/64)) tile
// co-visibility matrix, or nullptr for "dense".  Same workspace as the dense
// solve; falls back to the dense schedule when the structure offers nothing.
struct CholPlan;
CholPlan* chol_plan_create(int n, const uint8_t* adj);
// a rank's plan of a sharded solve (sparse_cholesky.hip): its private tile columns first, the shared ones above them
CholPlan* chol_plan_create_sharded(int n, const uint8_t* adj, const uint8_t* tile_class);
void chol_plan_solve_phase(const CholPlan* plan, int phase, double* A, int lda, double* b, double* work, double* fail_flag, hipStream_t st);
int chol_plan_split_level(const CholPlan* plan);
const std::vector<int>& chol_plan_shared_tiles(const CholPlan* plan);
void chol_plan_destroy(CholPlan* plan);
// zero the tiles of A the plan's assembly / factorisation touch; false = dense plan (the caller clears everything)
// tail / tail_count: a vector of doubles to zero in the same launch (null / 0: none)
bool chol_plan_clear(const CholPlan* plan, double* A, int lda, hipStream_t st, double* tail = nullptr, size_t tail_count = 0);
// S <- D S D, rhs <- D rhs, gc <- D gc, colsq <- D^2 colsq over the tiles chol_plan_clear clears (D = diag(s), n entries)
void chol_plan_rescale(const CholPlan* plan, double* A, int lda, int n, const double* s, double* rhs, double* colsq, double* gc, hipStream_t st);
// For a caller that clears and mirrors inside launches of its own (sparse plan only; nzero = 0 otherwise):
// zero_items: {r0, h, c0, w} (device) of the tiles k_sp_symm writes followed by the tiles chol_plan_clear zeroes -- every tile
// of A a solve on the plan reads or writes; symm_map[tr * nt + tc] != 0 (device): the lower tile (tr, tc) is mirrored
// into (tc, tr) before the factorisation (what k_sp_symm does; a caller that writes both entries itself on a buffer whose
// zero_items are clear leaves the bytes k_sp_symm leaves).
struct CholTileLists { const int* zero_items; int nzero; const int* symm_map; int nt; };
CholTileLists chol_plan_tile_lists(const CholPlan* plan);
int chol_plan_levels(const CholPlan* plan);
double chol_plan_flops(const CholPlan* plan);   // FP64 flops of one solve on the plan (n^3 / 3 for the dense schedule)
void chol_plan_solve(const CholPlan* plan, double* A, int lda, double* b, double* work, double* fail_flag, hipStream_t st);

#ifdef __HIPCC__
// The LM diagonal on a diagonal entry of the reduced system (sv: the assembled entry, cv: the squared column norm) and the
// entry's share of the gradient max-norm (gv: gradient entry, sr: Jacobi scale): one definition for k_finalize_rcs and
// for the k_schur_sum that does its work, so the two produce the same bits
__device__ __forceinline__ double lm_diag_entry(double sv, double cv, double radius) { return sv + fmin(fmax(cv, 1e-6), 1e32) / radius; }
__device__ __forceinline__ double lm_grad_entry(double gv, double sr) { return fabs(gv / sr); }
// DevProblem::lm_cur: does this launch take its state / candidate buffers the other way round?  (a scalar load, uniform)
__device__ __forceinline__ bool lm_flip(const DevProblem& P) { return P.lm_cur != nullptr && *P.lm_cur != 0; }
// one {r0, h, c0, w} tile item of a CholPlan list zeroed by the calling workgroup
__device__ __forceinline__ void clear_tile_item(double* __restrict__ A, int lda, const int* __restrict__ it) {
  const int r0 = it[0], h = it[1], c0 = it[2], w = it[3];
  for (int e = threadIdx.x; e < 64 * 64; e += blockDim.x) {
    const int r = e >> 6, c = e & 63;
    if (r < h && c < w) A[(size_t)(r0 + r) * lda + c0 + c] = 0.0;
  }
}
// Workgroup b of nb (256 threads) folds its contiguous slice of the per-tile partials into out[b][nfields]: the first stage
// of the two-stage reduction (k_reduce_tiles_stage1, and the launches that carry it as extra workgroups)
__device__ __forceinline__ void reduce_tiles_stage1_body(int ntiles, const double* __restrict__ part, int nfields,
                                                         const int* __restrict__ fmaxflag, double* __restrict__ out, int b, int nb,
                                                         double (*sm)[4]) {
  const int per = (ntiles + nb - 1) / nb;
  const int t0 = b * per, t1 = min(ntiles, t0 + per);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double acc[8];
  bool ismax[8];
#pragma unroll
  for (int f = 0; f < 8; ++f) { acc[f] = 0.0; ismax[f] = f < nfields && fmaxflag[f] != 0; }
  for (int t = t0 + (int)threadIdx.x; t < t1; t += 256) {
    const double* row = part + (size_t)t * nfields;
#pragma unroll
    for (int f = 0; f < 8; ++f)
      if (f < nfields) { const double v = row[f]; acc[f] = ismax[f] ? fmax(acc[f], v) : acc[f] + v; }
  }
#pragma unroll
  for (int f = 0; f < 8; ++f) {
    if (f >= nfields) break;
    double v = acc[f];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_xor(v, off, 64); v = ismax[f] ? fmax(v, o) : v + o; }
    if (lane == 0) sm[f][wv] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < nfields) {
    const int f = threadIdx.x;
    double v = sm[f][0];
    for (int w = 1; w < 4; ++w) v = ismax[f] ? fmax(v, sm[f][w]) : v + sm[f][w];
    out[(size_t)b * nfields + f] = v;
  }
}
// Deterministic reduction of per-tile partials into a scalar block by ONE workgroup of 1024 threads:
// field f of tile t at part[t * nfields + f]; result -> scal[f2s[f]] (sum, or max if fmaxflag[f]).
// Every thread folds its tiles for all fields, a wave shuffle tree per field, the 16 wave results are combined
// in wave order.  Ends with a workgroup barrier: the scalars are visible to every thread afterwards.
__device__ __forceinline__ void reduce_tiles_body(int ntiles, const double* __restrict__ part, int nfields,
                                                  const int* __restrict__ f2s, const int* __restrict__ fmaxflag,
                                                  double* __restrict__ scal, double (*sm)[16], bool atomic_max = false) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double acc[8];
  bool ismax[8];
#pragma unroll
  for (int f = 0; f < 8; ++f) { acc[f] = 0.0; ismax[f] = f < nfields && fmaxflag[f] != 0; }
  // four tiles per thread and step, all loads (clamped, unconditional) in flight before the first use;
  // the accumulation order of a thread is unchanged (t, t + 1024, t + 2048, ...)
  for (int t0 = threadIdx.x; t0 < ntiles; t0 += 4096) {
    double v[4][8];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double* row = part + (size_t)min(t0 + 1024 * u, ntiles - 1) * nfields;
#pragma unroll
      for (int f = 0; f < 8; ++f) v[u][f] = row[min(f, nfields - 1)];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (t0 + 1024 * u >= ntiles) break;
#pragma unroll
      for (int f = 0; f < 8; ++f)
        if (f < nfields) acc[f] = ismax[f] ? fmax(acc[f], v[u][f]) : acc[f] + v[u][f];
    }
  }
#pragma unroll
  for (int f = 0; f < 8; ++f) {
    if (f >= nfields) break;
    double v = acc[f];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_xor(v, off, 64); v = ismax[f] ? fmax(v, o) : v + o; }
    if (lane == 0) sm[f][wv] = v;
  }
  __syncthreads();
  if (threadIdx.x < (unsigned)nfields) {
    const int f = threadIdx.x;
    double v = sm[f][0];
    for (int w = 1; w < 16; ++w) v = ismax[f] ? fmax(v, sm[f][w]) : v + sm[f][w];
    // atomic_max: other workgroups of the same launch fold their own maxima into the same scalar (non-negative values: the
    // IEEE bit patterns order like the numbers; a maximum does not depend on the order of its operands)
    if (ismax[f] && atomic_max) { if (v == v) atomicMax(reinterpret_cast<unsigned long long*>(&scal[f2s[f]]), (unsigned long long)__double_as_longlong(v)); }
    else if (ismax[f]) scal[f2s[f]] = fmax(scal[f2s[f]], v);
    else scal[f2s[f]] += v;
  }
  __threadfence_block();
  __syncthreads();
}
#endif

}  // namespace thip
