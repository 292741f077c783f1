// ba_handle.h -- what the translation units of the BA handle API share (ba_plan.hip: create; ba_solver.hip: the LM side;
// ba_query.hip: evaluate, covariance, reduced system; ba_covariance.hip: the covariance of the coupled problem): the pinned staging arena and the pooled device buffer, the handle
// itself, the host threading of its passes, the device-resident LM state, and the handle-level functions of ba_solver.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "ba_kernels.h"
#include "device_util.h"
#include "pools.h"
#include "host_team.h"

namespace thip {
inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// Small pageable sources (the ~60 index / flag vectors of a create()) are copied into pinned blocks that live until the
// end of the call, so that their uploads queue behind the big ones instead of each waiting for the stream: a create() at
// 3 M observations spent ~5 ms in those waits -- the DMA of the 72 MB of sorted observations in front of them -- while the
// host had the K3 plan and the gather lists still to build.  The arena belongs to the handle: create() returns without waiting
// for the uploads (everything else on the handle queues behind them on its stream); the blocks go back to the host cache at the
// end of the first run() -- which has waited for the stream -- or with the handle, whose destructor waits for it.
struct StageArena {
  std::vector<std::unique_ptr<HBuf<char>>> blocks;
  size_t used = 0;
  hipStream_t stream = nullptr;
  void release() { blocks.clear(); used = 0; }   // (after a synchronisation of the stream)
  void* reserve(size_t bytes) {   // room for `bytes` in a pinned block (the caller fills it); nullptr: the caller uploads from its source and waits
    if (getenv("THEIA_HIP_NO_PINNED")) return nullptr;   // (test switch: a host that refuses to pin memory)
    const size_t al = (bytes + 63) & ~(size_t)63;
    if (blocks.empty() || used + al > blocks.back()->cap) {
      std::unique_ptr<HBuf<char>> b(new HBuf<char>);
      if (!b->reserve(std::max<size_t>(al, (size_t)4 << 20))) return nullptr;
      blocks.push_back(std::move(b)); used = 0;
    }
    void* dst = blocks.back()->p + used;
    used += al;
    return dst;
  }
  void* put(const void* src, size_t bytes) {
    void* dst = reserve(bytes);
    if (dst) std::memcpy(dst, src, bytes);
    return dst;
  }
};
inline StageArena*& stage_arena() { static thread_local StageArena* a = nullptr; return a; }
struct StageScope {   // the arena (the handle's: it lives until the uploads are known to be done) serves this thread's uploads
  StageArena* prev;
  explicit StageScope(StageArena* a) : prev(stage_arena()) { stage_arena() = a; }
  ~StageScope() { stage_arena() = prev; }
  StageScope(const StageScope&) = delete;
  StageScope& operator=(const StageScope&) = delete;
};

template <typename T>
struct PoolBuf {
  // Blocks come from the library's device cache (pools.h): creating a handle makes ~80 allocations, and at a million
  // observations hipMalloc + hipFree were ~15 ms of a 100 ms create().  A cached block is handed out without a device
  // synchronisation, so the owner makes sure no kernel still uses a buffer when it goes back (the handle's destructor
  // waits for its stream; a re-allocation waits for the device).
  T* p = nullptr;
  size_t n = 0, bytes = 0;
  PoolBuf() = default;
  PoolBuf(const PoolBuf&) = delete;
  PoolBuf& operator=(const PoolBuf&) = delete;
  ~PoolBuf() { if (p) dev_pool().give(p, bytes); }
  void swap(PoolBuf& o) { std::swap(p, o.p); std::swap(n, o.n); std::swap(bytes, o.bytes); }   // the two buffers change owners
  int alloc(size_t count) {
    if (p) { (void)hipDeviceSynchronize(); dev_pool().give(p, bytes); p = nullptr; bytes = 0; }
    n = count;
    if (count == 0) return 0;
    size_t got = 0;
    p = static_cast<T*>(dev_pool().take(std::max<size_t>(count * sizeof(T), 256), &got));
    if (!p) { n = 0; return set_error(THEIA_HIP_ERR_OUT_OF_MEMORY, "hipMalloc(%zu) failed", count * sizeof(T)); }
    bytes = got;
    return 0;
  }
  int upload(const std::vector<T>& h, hipStream_t st) { return upload(h.data(), h.size(), st, false); }
  // pinned = the source is a pinned block that outlives the copy (the caller synchronises the stream before it lets go)
  int upload(const T* src, size_t count, hipStream_t st, bool pinned) {
    int rc = alloc(count);
    if (rc) return rc;
    // A pageable source (usually a temporary vector) must have been read before upload() returns.
    if (count) {
      StageArena* a = stage_arena();
      if (!pinned && a && a->stream == st && count * sizeof(T) <= ((size_t)32 << 20))
        if (const void* staged = a->put(src, count * sizeof(T))) { src = static_cast<const T*>(staged); pinned = true; }
      HIP_TRYR(hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, st));
      if (!pinned) HIP_TRYR(hipStreamSynchronize(st));
    }
    return 0;
  }
};

}  // namespace thip

using namespace thip;   // (an internal header: its includers speak of the library's own names unqualified)
struct theia_ba_handle_s {
  theia_ba_options opt;
  void* idh = nullptr;   // inverse-depth problems (THEIA_BA_FLAG_INVERSE_DEPTH) live in their own object (ba_invdepth.hip): create / reset / run / download only
  int nc = 0, ng = 0, np = 0, ncv = 0, n = 0, pd = 3;
  int64_t nobs = 0, nobs_main = 0;
  int ntiles_main = 0, ntiles_eval = 0, ntiles_all = 0;  // linearize tiles < + long-track eval tiles < + fixed tiles
  int long_nobs = 0, long_ntracks = 0;
  PoolBuf<int> long_obs_index, long_obs_slot, long_track_start, long_track_pt;
  PoolBuf<double> long_scratch;
  hipStream_t stream = nullptr;
  static constexpr int kMaxChunk = 8;   // LM iterations enqueued per host synchronisation
  hipEvent_t ev[kMaxChunk][6] = {};
  PoolBuf<char> lm_state;                // LmState (device): radius, cost, counters, termination; then the trace head (kLmBlockBytes)
  PoolBuf<char> lm_ctl;                  // LmCtl (device): per-run tolerances, caps, trace pointers
  hipGraph_t graph = nullptr;           // one captured LM iteration (no all-reduce callback, no phase timing)
  hipGraphExec_t graph_exec = nullptr;
  bool graph_failed = false;
  void drop_graph() {
    if (graph_exec) { (void)hipGraphExecDestroy(graph_exec); graph_exec = nullptr; }
    if (graph) { (void)hipGraphDestroy(graph); graph = nullptr; }
  }
  PoolBuf<double> tr_tail;               // trace entries kTraceHead .. of the five arrays (LmCtl::tt), allocated when asked for
  size_t tr_tail_cap = 0;                // entries per array
  // host-side bookkeeping
  HBuf<int64_t> perm;              // sorted obs index -> original obs index (a block of the pinned host cache: no page faults)
  std::vector<int> cam_red, grp_red, grp_k;
  // cameras that take part in the fused Schur assembly: a variable extrinsics block OR (fused_bw > 0) a variable intrinsics
  // group.  cam_part[c] = index among them in camera order (-1 = none), part_cam = inverse.  Without variable intrinsics
  // this is cam_red.
  std::vector<int> cam_part, part_cam;
  int ncp = 0, fused_bw = 0, n_sum_items2 = 0;
  unsigned fused_kmask = 0;
  std::vector<unsigned> grp_free;
  std::vector<uint8_t> cam_mask, pt_const;
  int ni = 0, ngv = 0;
  // device buffers
  PoolBuf<double> snap_cam, snap_pts, snap_intr;   // theia_hip_ba_snapshot_parameters
  PoolBuf<double> xnorm_part;
  bool has_snapshot = false;
  PoolBuf<double> cam[2], pts[2], intr[2], scale_c, scale_p, ones_c, ones_p, colsq_c0, colsq_p0;
  PoolBuf<double> scale_i, ones_i, colsq_i0, scale_red;
  PoolBuf<int> d_grp_red, d_grp_k;
  PoolBuf<unsigned> d_grp_free, d_red_free;
  int intr_rows = 10;            // intrinsics rows per gather record (ba_kernels.hip RecI): 10, or 4 compact rows
  PoolBuf<int> group_model, cam_group, d_cam_red, obs_cam, obs_pt, tile_start, tile_count, f2s, fmaxflag;
  PoolBuf<uint8_t> d_cam_mask, d_pt_const;
  PoolBuf<double2> obs_uv, obs_si;
  PoolBuf<uint8_t> obs_kind;
  PoolBuf<double> reduce, Vinv, gp, tile_part, red_part, scalB, chol_work, stop_flag;
  PoolBuf<double> rec;                       // per-observation records of the gather-based Schur assembly
  PoolBuf<int> diag_items, cam_obs, blk_items, slot_obs, slot_pt;
  PoolBuf<int> prior_cam, prior_kind;        // camera priors in use (compact list)
  // inner iterations (ba_inner.hip): observation lists by camera / group / track, a third parameter buffer the sweep
  // works on, its scalars {step^2, |x|^2, cost, invalid}, the gate flag
  bool inner = false;
  PoolBuf<int> in_cam_off, in_cam_idx, in_grp_off, in_grp_idx, in_trk_off, in_gate, in_grp_bar;
  PoolBuf<double> in_grp_part;   // partial sums of the intrinsics sweep, inner_group_wgs() workgroups per group
  PoolBuf<double> in_cam, in_pts, in_intr, in_scal, in_part;
  // inner iterations of a SHARDED solve (theia_hip_ba_set_inner_global): every rank sweeps all cameras and intrinsics groups
  // over the FULL observation set (the same sums on every rank: no exchange of their results), its own tracks afterwards
  bool inner_global = false;
  int g_np = 0, g_npriors = 0;
  int64_t g_nobs = 0;
  PoolBuf<double2> g_uv, g_si;
  PoolBuf<int> g_cam, g_pt, g_cam_off, g_cam_idx, g_grp_off, g_grp_idx, g_pidx, g_prior_cam, g_prior_kind;
  PoolBuf<uint8_t> g_kind;
  PoolBuf<double> g_pts, g_prior_vec, g_prior_info, g_stage;
  int in_ntracks = 0;
  PoolBuf<double> prior_vec, prior_info;
  int n_priors = 0;
  PoolBuf<int2> blk_pairs;
  PoolBuf<int> pt_sum_slot;   // [np] pseudo-record of a track's summed intrinsics fields, -1 = none (build_gather_lists_intr)
  PoolBuf<uint8_t> slot_in_sum;   // [#records] the observation's track is summed
  PoolBuf<uint8_t> pt_sum_cnt;    // [np] number of summed groups (pseudo-records) of a track
  PoolBuf<int> sum_group;         // [#pseudo-records] reduced group index
  int sum_base = 0;              // first pseudo-record slot
  int n_trk_sums = 0;
  int n_diag_items = 0, n_blk_items = 0;
  // fused linearise + Schur plan (ba_fused.hip)
  bool use_fused = false;
  unsigned model_mask = 0xffu;          // camera models present in the problem
  PoolBuf<FusedRun> fruns;
  PoolBuf<int> frun_cams, frun_stage, tile_trk_end, sum_items, sum_src, frun_order, frun_next;
  PoolBuf<unsigned short> frun_tgt;
  PoolBuf<uint8_t> obs_lc, obs_tl;
  PoolBuf<double> fpart, camrot, camrot_cand, camdir;
  int n_fruns = 0, n_sum_items = 0;
  bool sum_covers_n = false;   // every row of the reduced system belongs to a camera with a diagonal item of sum_items
  double* h_scal = nullptr;  // pinned: [scalA(16) | scalB(16) | stop flag out / in (2) | spare]
  char* h_state = nullptr;   // pinned: read-back of lm_state (kLmBlockBytes)
  int cur = 0;
  bool have_scale = false;
  bool camrot_valid = false;     // P.camrot holds the per-camera blocks of the current state (k_lm_accept keeps it so on accepted steps)
  double fixed_cost = 0.0;
  theia_allreduce_fn allreduce = nullptr;
  void* allreduce_ctx = nullptr;
  ReduceBuf rb;
  DevProblem P;
  // K3 schedule: tile co-visibility of the reduced system (this rank's tracks;
  // OR-ed over the ranks before the first distributed solve) and its plan
  std::vector<uint8_t> tile_adj;
  CholPlan* plan = nullptr;
  bool plan_is_global = true;
  // multi-rank: only the structurally non-zero lower 64x64 tiles of S travel through the all-reduce
  PoolBuf<int2> pack_tiles;
  PoolBuf<double> pack_buf;
  int shard_rank = -1, shard_world = 0;   // theia_hip_ba_set_shard
  // distributed K3 of a sharded solve (sync_plan): every rank factors the tile columns only its own tracks touch before the
  // all-reduce, which then carries the shared tiles only; tile_cls: 0 shared, 1 this rank's, 2 another rank's
  bool dist_k3 = false;
  std::vector<uint8_t> tile_adj_local, tile_cls, tile_touch;   // tile_touch: this rank's observations / priors write into the tile column
  PoolBuf<uint8_t> d_tile_cls;
  int n_pack_tiles = 0;

  StageArena stage;                     // pinned staging of create()'s small uploads (released after the first run)

  ~theia_ba_handle_s() {
    if (idh) thip::id_handle_destroy(idh);
    if (stream) (void)hipStreamSynchronize(stream);   // the buffers below go back to the device cache, not to hipFree
    drop_graph();
    if (plan) chol_plan_destroy(plan);
    for (auto& row : ev) for (auto& e : row) if (e) (void)hipEventDestroy(e);
    if (h_scal) (void)hipHostFree(h_scal);
    if (h_state) (void)hipHostFree(h_state);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

namespace thip {
// Host-side loops over independent index ranges on a few threads (handle creation at millions of observations); host_thread_cap() caps them.
inline thread_local bool g_in_host_region = false;
// fn(k) for the parts k = 0 .. nparts-1 of a fixed partition (the result must not depend on who runs which part)
template <class F>
void host_parts(int nparts, bool threaded, F&& fn) {
  bool& in_region = g_in_host_region;   // a region started inside a region runs on its caller alone
  const unsigned cap = (threaded && !in_region) ? std::min<unsigned>(host_thread_cap(), (unsigned)nparts) : 1u;
  if (cap <= 1) { for (int k = 0; k < nparts; ++k) fn(k); return; }
  struct Flag { bool& f; explicit Flag(bool& x) : f(x) { f = true; } ~Flag() { f = false; } };
  host_for(nparts, cap, [&fn](int k) { Flag g(g_in_host_region); fn(k); });
}
template <class F>
void host_chunks(int64_t n, F&& fn) {
  const unsigned cap = host_thread_cap();
  // (THEIA_HIP_HOST_CHUNK_MIN: test switch -- small problems through the threaded passes)
  const char* cm = getenv("THEIA_HIP_HOST_CHUNK_MIN");
  const int64_t min_n = cm ? std::max(1, atoi(cm)) : 262144;
  if (n < min_n || cap <= 1) { fn((int64_t)0, n); return; }
  const int64_t per = (n + cap - 1) / cap;
  host_parts((int)cap, true, [&](int t) {
    const int64_t a = std::min<int64_t>(n, (int64_t)t * per), b = std::min<int64_t>(n, a + per);
    if (a < b) fn(a, b);
  });
}
// number of parts of a threaded pass over n items, `grain` items per part at least (the test switch lowers the grain)
inline int host_part_count(int64_t n, int64_t grain) {
  const char* cm = getenv("THEIA_HIP_HOST_CHUNK_MIN");
  if (cm) grain = std::max<int64_t>(1, std::min<int64_t>(grain, atoi(cm)));
  return (int)std::max<int64_t>(1, std::min<int64_t>(host_thread_cap(), n / grain));
}
enum { SB_COST = 0, SB_MCC = 1, SB_STEPSQ = 2, SB_XNORMSQ = 3, SB_INVALID = 4, SB_STEPSQ_CAM = 8, SB_XNORMSQ_CAM = 9 };

// ------------------------------------------------------------ LM step control
// Trust-region bookkeeping of one solve, resident on the device so that several
// iterations can be enqueued without a host round trip.
struct LmState {
  double radius, decrease_factor, x_cost, x_norm, gmax, minimum_cost, initial_cost;
  int step_successful, iter, invalid_steps, term, done, first, accepted, num_successful, trace_size, pending_grad,
      fail_at_first, bodies;
  int inner_enabled;   // inner iterations still running (they switch themselves off: inner_iteration_tolerance)
  int use_inner;       // this body's candidate is the point the inner iterations ended at (k_lm_accept copies that one)
  int cur;             // the folded LM chain: the parameter buffers that hold the state (0 or 1), flipped by k_reduce_control on an accepted step
};
// The five trace arrays (cost, gradient max norm, step norm, radius, accepted) are cut in two: entries [0, kTraceHead) sit
// right behind the LmState, so that the read-back of the state every chunk of iterations ends with brings them along and a
// solve whose trace fits needs no copy of its own; the entries beyond are one block (LmCtl::tt), copied after the loop.
constexpr int kTraceHead = 64;
constexpr size_t kLmStateBytes = 256;                                            // offset of the trace head in lm_state / h_state
constexpr size_t kLmBlockBytes = kLmStateBytes + 5 * sizeof(double) * kTraceHead;
static_assert(sizeof(LmState) <= kLmStateBytes, "the trace head would overlap the state");
struct LmCtl {   // per-run control block, device resident so that a captured graph of the iteration stays valid
  int max_iterations, trace_capacity;
  double function_tolerance, gradient_tolerance, parameter_tolerance, max_radius, fixed_cost;
  double* th;          // trace head [5][kTraceHead] (array 4 holds ints), null = no trace
  double* tt;          // trace tail [5][tt_cap]: entry k >= kTraceHead of array a at tt[a * tt_cap + k - kTraceHead]
  int tt_cap;
  const double* inner_scal;   // [4] = {|x - x_inner|^2, |x_inner|^2, cost at x_inner, invalid}, null = no inner iterations
};
// entry k of trace array a (0 cost, 1 gradient, 2 step, 3 radius; 4 accepted: reinterpret as int*, int index k)
__host__ __device__ inline double* lm_trace_array(const LmCtl& c, int a, int k, int* idx) {
  if (k < kTraceHead) { *idx = k; return c.th + (size_t)a * kTraceHead; }
  *idx = k - kTraceHead;
  return c.tt + (size_t)a * c.tt_cap;
}

// the handle-level functions of ba_solver.hip
int validate(const theia_ba_problem* p, const theia_ba_options* o);
void fill_devproblem(theia_ba_handle_s* h);
int upload_parameters(theia_ba_handle_s* h, const theia_ba_problem* p);
void release_stage_if_idle(theia_ba_handle_s* h);
int do_allreduce(theia_ba_handle_s* h, double* buf, size_t count, int op);
int cost_of_tiles(theia_ba_handle_s* h, int tile0, int ntiles, const double* cam, const double* pts, double* cost, double* invalid);
int compute_scale(theia_ba_handle_s* h);
bool scale_fold_applies(const theia_ba_handle_s* h);
bool lm_glue_applies(const theia_ba_handle_s* h);
bool lm_glue_run(const theia_ba_handle_s* h);   // ... and the handle's options and the environment let run() take it
// What a body of run() launches between its large kernels: LM_SEPARATE the glue kernels in launches of their own and
// k_lm_accept; LM_FOLD_FIRST the first body of a run where lm_glue_run(): the same launches, but it clears the reduced system
// behind itself and an accepted step flips LmState::cur instead of the copy; LM_FOLDED the bodies after it: no clear on entry,
// k_schur_sum finishes the system, no k_sp_symm, k_cam_update finishes the scalars and clears
enum LmChain { LM_SEPARATE = 0, LM_FOLD_FIRST = 1, LM_FOLDED = 2 };
int enqueue_linearize(theia_ba_handle_s* h, int slot = 0, bool first_fold = false, LmChain chain = LM_SEPARATE);
int enqueue_solve_and_backsub(theia_ba_handle_s* h, int slot = 0, bool defer_reduce = false, LmChain chain = LM_SEPARATE);
int sync_plan(theia_ba_handle_s* h);
void debug_sticky(const char* where);

}  // namespace thip
