// ba_solver.hip -- the Levenberg-Marquardt side of the BA C-ABI (include/theia_hip.h): the control loop that replaces
// ceres::Solve as configured by
//   BundleAdjuster::SetSolverOptions / Optimize
//   (src/theia/sfm/bundle_adjustment/bundle_adjuster.cc:63-89,315-355),
// its control kernels, and the handle-level helpers the other BA files call (declared in ba_handle.h).  The handle is built
// in ba_plan.hip; the entry points that only read one are in ba_query.hip.
// LM rules restated from Ceres 2.2 (trust_region_minimizer.cc,
// levenberg_marquardt_strategy.cc): see DESIGN.md "LM control".
// All state stays in HBM, including the trust-region step control (k_lm_control):
// the host enqueues several LM iterations back to back and synchronises once
// per chunk to read the LM state.
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <limits>

#include "ba_handle.h"
#include "ba_host_rules.h"
#include "lm_rules.h"

namespace lm = thip::lm;

namespace {

__device__ void lm_trace(LmState* st, const LmCtl& c, double cost, double g, double step, double radius, int acc) {
  if (!c.th || st->trace_size >= c.trace_capacity) return;
  const int k = st->trace_size++;
  int i;
  lm_trace_array(c, 0, k, &i)[i] = cost; lm_trace_array(c, 1, k, &i)[i] = g; lm_trace_array(c, 2, k, &i)[i] = step;
  lm_trace_array(c, 3, k, &i)[i] = radius; reinterpret_cast<int*>(lm_trace_array(c, 4, k, &i))[i] = acc;
}

// One pass of the TrustRegionMinimizer loop body (ceres trust_region_minimizer.cc; the
// same rules the host loop of the first versions applied after each read-back):
// sa = scalars of the linearisation at x, sb = scalars of the trial step.
// (sa carries no __restrict__: on the folded chain k_reduce_control clears those scalars itself afterwards, through another pointer)
__device__ void lm_control_body(LmState* st, const double* sa, const double* __restrict__ sb,
                                const LmCtl* __restrict__ cp) {
  const LmCtl c = *cp;
  st->accepted = 0; st->use_inner = 0;
  if (st->done) return;
  st->bodies++;
  const double x_cost = sa[SC_COST];
  const double gmax = sa[SC_GMAX];
  st->x_cost = x_cost; st->gmax = gmax;
  if (st->pending_grad >= 0 && c.th) { int i; lm_trace_array(c, 1, st->pending_grad, &i)[i] = gmax; }
  st->pending_grad = -1;
  if (st->first) {
    st->first = 0;
    st->initial_cost = x_cost + c.fixed_cost;
    st->minimum_cost = x_cost;
    if (sa[SC_INVALID] > 0.0 || !isfinite(x_cost)) { st->term = THEIA_TERM_FAILURE; st->fail_at_first = 1; st->done = 1; return; }
    lm_trace(st, c, x_cost + c.fixed_cost, gmax, 0.0, st->radius, 1);
  }
  if (st->iter >= c.max_iterations) { st->term = THEIA_TERM_NO_CONVERGENCE; st->done = 1; return; }
  if (lm::converged_before_step(*st, gmax, c.gradient_tolerance)) { st->term = THEIA_TERM_CONVERGENCE; st->done = 1; return; }
  st->iter++;
  double mcc = sb[SB_MCC];
  double stepsq = sb[SB_STEPSQ] + sb[SB_STEPSQ_CAM];
  const bool solved = sa[SC_NOTPD] == 0.0 && isfinite(mcc) && isfinite(stepsq);
  if (!(solved && mcc > 0.0)) {
    if (!lm::invalid_step(*st)) { st->term = THEIA_TERM_FAILURE; st->done = 1; return; }
    lm_trace(st, c, x_cost + c.fixed_cost, gmax, 0.0, st->radius, 0);
    return;
  }
  lm::valid_step(*st);
  double cand_cost = sb[SB_COST];
  if (sb[SB_INVALID] > 0.0 || !isfinite(cand_cost)) cand_cost = DBL_MAX;
  // TrustRegionMinimizer::DoInnerIterationsIfNeeded: the sweep ran on a copy of the candidate (k_inner_gate said so
  // from the same quantities); its result replaces the candidate unless the evaluation there failed
  bool inner_useful = false;
  double xnormsq = sb[SB_XNORMSQ] + sb[SB_XNORMSQ_CAM];
  if (c.inner_scal && st->inner_enabled && cand_cost < DBL_MAX) {
    const double inner_cost = c.inner_scal[2];
    if (c.inner_scal[3] == 0.0 && isfinite(inner_cost)) {
      st->use_inner = 1;
      mcc += cand_cost - inner_cost;
      inner_useful = inner_cost < x_cost;
      st->inner_enabled = (1.0 - inner_cost / cand_cost) > 1e-3;   // inner_iteration_tolerance
      cand_cost = inner_cost;
      stepsq = c.inner_scal[0]; xnormsq = c.inner_scal[1];
    }
  }
  const double step_norm = sqrt(stepsq);
  if (lm::parameter_rule(step_norm, st->x_norm, c.parameter_tolerance)) {
    lm_trace(st, c, cand_cost + c.fixed_cost, gmax, step_norm, st->radius, 0);
    st->term = THEIA_TERM_CONVERGENCE; st->done = 1; return;
  }
  const double cost_change = x_cost - cand_cost;
  if (lm::function_rule(x_cost, cand_cost, c.function_tolerance)) {
    lm_trace(st, c, cand_cost + c.fixed_cost, gmax, step_norm, st->radius, 0);
    st->term = THEIA_TERM_CONVERGENCE; st->done = 1; return;
  }
  const double rho = cost_change / mcc;
  if (inner_useful || lm::step_accepted(rho)) {   // IsStepSuccessful
    st->accepted = 1;   // k_lm_accept copies the candidate buffers over the state (or k_reduce_control makes the buffers change roles)
    st->x_norm = sqrt(xnormsq);
    lm::accept<true>(*st, rho, c.max_radius);   // pow, as the oracle
    st->num_successful++;
    if (cand_cost < st->minimum_cost) st->minimum_cost = cand_cost;
    if (c.th && st->trace_size < c.trace_capacity) st->pending_grad = st->trace_size;
    lm_trace(st, c, cand_cost + c.fixed_cost, -1.0, step_norm, st->radius, 1);
  } else {
    lm::shrink(*st);
    lm_trace(st, c, cand_cost + c.fixed_cost, gmax, step_norm, st->radius, 0);
  }
  // the iteration cap is known now: no further pass is needed to detect it
  if (st->iter >= c.max_iterations) { st->term = THEIA_TERM_NO_CONVERGENCE; st->done = 1; }
}

__global__ void k_lm_control(LmState* st, const double* __restrict__ sa, const double* __restrict__ sb,
                             const LmCtl* __restrict__ cp) {
  lm_control_body(st, sa, sb, cp);
}
// The trace entry of an accepted step waits for the gradient at the accepted point, which the next body's linearisation
// brings (pending_grad).  A solve that ends with that step has no next body: run() linearises once more and this fills it.
__global__ void k_lm_pending_gradient(LmState* st, const double* __restrict__ sa, const LmCtl* __restrict__ cp) {
  const LmCtl c = *cp;
  if (st->pending_grad >= 0 && c.th) { int i; lm_trace_array(c, 1, st->pending_grad, &i)[i] = sa[SC_GMAX]; }
  st->pending_grad = -1;
}
// The tile reduction of the trial step (launch_reduce_tiles cfg 1 -> scalB) and the step control in one launch.
// clear16 (the folded LM chain, lm_glue_applies): an accepted step flips LmState::cur instead of the copy of k_lm_accept, and
// the scalars of the linearisation are cleared once the control body has read them
// -- the next k_schur_sum and K3 need SC_GMAX and SC_NOTPD at zero, the sums land on zeros; the vectors in front of them
// (rhs | colsq | gc) need no clear there: k_schur_sum writes every entry (theia_ba_handle_s::sum_covers_n).
__global__ __launch_bounds__(1024) void k_reduce_control(int ntiles, const double* __restrict__ part,
                                                         const int* __restrict__ f2s, const int* __restrict__ fmaxflag,
                                                         LmState* st, const double* sa, double* __restrict__ sb,
                                                         const LmCtl* __restrict__ cp, double* __restrict__ clear16, int flip) {
  __shared__ double sm[8][16];
  thip::reduce_tiles_body(ntiles, part, 5, f2s, fmaxflag, sb, sm);
  if (threadIdx.x == 0) {
    lm_control_body(st, sa, sb, cp);
    if (flip && st->accepted) st->cur ^= 1;   // an accepted step: state and candidate buffers change roles (never after done)
  }
  if (clear16) {
    __syncthreads();   // the control body has read the scalars
    if (threadIdx.x < 16) clear16[threadIdx.x] = 0.0;
  }
}

// |x| over the variable parameter blocks (TrustRegionMinimizer's x_norm at the start):
// out2[0] = points (per track shard), out2[1] = cameras + intrinsics.  kXnormBlocks workgroups write their
// partial sums to part[b][2]; k_xnorm_reduce adds them in block order (no atomics: the norm is reproducible).
constexpr int kXnormBlocks = 64;
constexpr int kMaxShardSlots = 1024;   // ranks whose MAX scalar fits in the packed SUM all-reduce
__global__ __launch_bounds__(256) void k_xnorm_partial(DevProblem P, const double* __restrict__ cam,
                                                       const double* __restrict__ pts, const double* __restrict__ intr,
                                                       double* __restrict__ part) {
  __shared__ double s1[256], s2[256];
  double sp = 0.0, sc = 0.0;
  const int t0 = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
  for (int p = t0; p < P.np; p += stride) {
    const double4 x = reinterpret_cast<const double4*>(pts)[p];   // unconditional load, masked sum
    const double m = P.pt_const[p] ? 0.0 : 1.0;
    sp += m * (((x.x * x.x + x.y * x.y) + x.z * x.z) + x.w * x.w);
  }
  if (blockIdx.x == 0) {
    for (int c = threadIdx.x; c < P.nc; c += 256)
      if (P.cam_red[c] >= 0) for (int q = 0; q < 6; ++q) sc += cam[6 * c + q] * cam[6 * c + q];
    if (P.ni)
      for (int g = threadIdx.x; g < P.ng_total; g += 256)
        if (P.grp_red[g] >= 0) for (int q = 0; q < P.grp_k[g]; ++q) sc += intr[(size_t)g * THEIA_MAX_INTRINSICS + q] * intr[(size_t)g * THEIA_MAX_INTRINSICS + q];
  }
  s1[threadIdx.x] = sp; s2[threadIdx.x] = sc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) { s1[threadIdx.x] += s1[threadIdx.x + s]; s2[threadIdx.x] += s2[threadIdx.x + s]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = s1[0]; part[2 * blockIdx.x + 1] = s2[0]; }
}
__global__ void k_xnorm_reduce(const double* __restrict__ part, int nblocks, double* __restrict__ out2) {
  double a = 0.0, b = 0.0;
  for (int k = 0; k < nblocks; ++k) { a += part[2 * k]; b += part[2 * k + 1]; }
  out2[0] = a; out2[1] = b;
}
__global__ void k_xnorm_set(LmState* st, const double* __restrict__ in2) { st->x_norm = sqrt(in2[0] + in2[1]); }
// the two above in one launch (no all-reduce between them)
__global__ void k_xnorm_reduce_set(const double* __restrict__ part, int nblocks, double* __restrict__ out2, LmState* st) {
  double a = 0.0, b = 0.0;
  for (int k = 0; k < nblocks; ++k) { a += part[2 * k]; b += part[2 * k + 1]; }
  out2[0] = a; out2[1] = b;
  st->x_norm = sqrt(a + b);
}
// start of a solve: the initial state and the control block travel as kernel arguments, the trial-step scalars are cleared
__global__ void k_lm_init(LmState* st, LmState sv, LmCtl* ctl, LmCtl cv, double* __restrict__ scalB) {
  *st = sv; *ctl = cv;
  for (int q = 0; q < 16; ++q) scalB[q] = 0.0;
}

// Packed all-reduce buffer: [tiles (64x64, zero padded) | rhs | colsq | g_c | 8 scalars].  S outside the
// structurally non-zero tiles is zero on every rank, so only those tiles are summed across ranks
// (C2: 39 tiles = 1.3 MB instead of the 11.5 MB dense matrix).
__global__ __launch_bounds__(256) void k_pack_rcs(int n, const double* __restrict__ base, const int2* __restrict__ tiles,
                                                  int ntiles, double* __restrict__ pack, int to_pack, int rank,
                                                  int world) {
  const int b = blockIdx.x;
  if (b < ntiles) {
    const int r0 = tiles[b].x * 64, c0 = tiles[b].y * 64;
    double* pk = pack + (size_t)b * 4096;
    for (int e = threadIdx.x; e < 4096; e += 256) {
      const int r = r0 + (e >> 6), c = c0 + (e & 63);
      if (r < n && c < n) {
        double* s = const_cast<double*>(base) + (size_t)r * n + c;
        if (to_pack) pk[e] = *s; else *s = pk[e];
      } else if (to_pack) pk[e] = 0.0;
    }
    return;
  }
  // tail: everything after S in the reduce buffer up to the 8 sum-reduced scalars
  const size_t tail = (size_t)3 * n + 8;
  double* src = const_cast<double*>(base) + (size_t)n * n;
  double* pk = pack + (size_t)ntiles * 4096;
  for (size_t e = (size_t)(b - ntiles) * 256 + threadIdx.x; e < tail; e += (size_t)(gridDim.x - ntiles) * 256) {
    if (to_pack) pk[e] = src[e]; else src[e] = pk[e];
  }
  // the MAX-reduced scalar (gradient max-norm, >= 0) in one slot per rank of the SUM all-reduce
  if (world > 0 && b == ntiles && threadIdx.x == 0) {
    double* slots = pk + tail;
    double* gmax = src + (size_t)3 * n + SC_GMAX;   // scal = [.. | colsq | gc | scal[16]]
    if (to_pack) {
      for (int r = 0; r < world; ++r) slots[r] = (r == rank) ? *gmax : 0.0;
    } else {
      double m = 0.0;
      for (int r = 0; r < world; ++r) m = fmax(m, slots[r]);
      *gmax = m;
    }
  }
}

// distributed K3: after the back-substitution a rank holds the step of its own private columns and of the shared ones; the
// columns of other ranks' private tiles are zeroed, the shared ones kept on rank 0 only, and one SUM all-reduce of the n
// doubles (x + 0 is exact) gives every rank the whole camera step
__global__ void k_y_own(int n, double* __restrict__ y, const uint8_t* __restrict__ tile_cls, int rank) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= n) return;
  const int c = tile_cls[d >> 6];
  if (!(c == 1 || (c == 0 && rank == 0))) y[d] = 0.0;
}

// accepted step: the candidate parameters become the state
// Will this body's control pass run inner iterations?  The same conditions lm_control_body applies, from the same inputs.
__global__ void k_inner_gate(const LmState* __restrict__ st, const double* __restrict__ sa, const double* __restrict__ sb,
                             int* __restrict__ gate) {
  const double mcc = sb[SB_MCC], stepsq = sb[SB_STEPSQ] + sb[SB_STEPSQ_CAM], cand = sb[SB_COST];
  const bool valid = sa[SC_NOTPD] == 0.0 && isfinite(mcc) && isfinite(stepsq) && mcc > 0.0;
  *gate = (!st->done && st->inner_enabled && valid && sb[SB_INVALID] == 0.0 && isfinite(cand)) ? 1 : 0;
}

// use_inner: the accepted point is the one the inner iterations ended at (in_*), not the trust-region candidate
__global__ void k_lm_accept(const LmState* __restrict__ st, double* __restrict__ cam, const double* __restrict__ cand_cam, size_t ncam,
                            double* __restrict__ pts, const double* __restrict__ cand_pts, size_t npts,
                            double* __restrict__ intr, const double* __restrict__ cand_intr, size_t nintr,
                            const double* __restrict__ in_cam = nullptr, const double* __restrict__ in_pts = nullptr,
                            const double* __restrict__ in_intr = nullptr, double* __restrict__ camrot = nullptr,
                            const double* __restrict__ camrot_cand = nullptr, size_t ncamrot = 0) {
  if (!st->accepted) return;
  if (st->use_inner) { cand_cam = in_cam; cand_pts = in_pts; if (nintr) cand_intr = in_intr; }
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  // the candidate's per-camera blocks become the state's (enqueue_linearize then skips k_cam_prep); never with inner iterations
  if (camrot && !st->use_inner)
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < ncamrot; i += stride) camrot[i] = camrot_cand[i];
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npts; i += stride) pts[i] = cand_pts[i];
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < ncam; i += stride) cam[i] = cand_cam[i];
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nintr; i += stride) intr[i] = cand_intr[i];
}

int supported_model(int m) { return m >= THEIA_CAM_PINHOLE && m <= THEIA_CAM_ORTHOGRAPHIC; }

}  // namespace

namespace thip {

int validate(const theia_ba_problem* p, const theia_ba_options* o) {
  if (!p || !o) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null problem/options");
  if (p->num_cameras < 0 || p->num_points < 0 || p->num_obs < 0 || p->num_groups < 0)
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "negative sizes");
  if (p->num_obs >= (int64_t)1 << 31) return set_error(THEIA_HIP_ERR_UNSUPPORTED, "num_obs >= 2^31");
  if (p->num_obs > 0 && (!p->cam_ext || !p->intrinsics || !p->group_model || !p->cam_group || !p->points ||
                         !p->obs_uv || !p->obs_cam || !p->obs_pt))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null array in problem");
  for (int c = 0; c < p->num_cameras; ++c)
    if (p->cam_group[c] < 0 || p->cam_group[c] >= p->num_groups)
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "cam_group[%d] out of range", c);
  for (int g = 0; g < p->num_groups; ++g)
    if (!supported_model(p->group_model[g]))
      return set_error(THEIA_HIP_ERR_UNSUPPORTED, "camera model %d of group %d has no HIP kernel yet", p->group_model[g], g);
  {   // (on host threads at millions of observations; the first offender is reported whoever finds it)
    std::atomic<int64_t> first_bad{std::numeric_limits<int64_t>::max()};
    host_chunks(p->num_obs, [&](int64_t i0, int64_t i1) {
      for (int64_t i = i0; i < i1; ++i)
        if (p->obs_cam[i] < 0 || p->obs_cam[i] >= p->num_cameras || p->obs_pt[i] < 0 || p->obs_pt[i] >= p->num_points) {
          int64_t cur = first_bad.load();
          while (i < cur && !first_bad.compare_exchange_weak(cur, i)) {}
          return;
        }
    });
    if (first_bad.load() != std::numeric_limits<int64_t>::max())
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "observation %lld indexes out of range", (long long)first_bad.load());
  }
  if (o->intrinsics_to_optimize < 0 || o->intrinsics_to_optimize > THEIA_INTR_ALL)
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "invalid intrinsics_to_optimize bit mask");
  if (o->prior_mask < 0 || o->prior_mask > 7) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "invalid prior_mask");
  if (p->obs_kind) {
    bool any = false;
    for (int64_t i = 0; i < p->num_obs; ++i) {
      if (p->obs_kind[i] > THEIA_OBS_DEPTH_PRIOR) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "obs_kind[%lld] is not a THEIA_OBS_* value", (long long)i);
      any = any || p->obs_kind[i] == THEIA_OBS_DEPTH_PRIOR;
    }
    if (any && !p->obs_sqrt_info)
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "depth-prior rows need obs_sqrt_info (1 / sqrt(depth_prior_variance))");
    if (any && !(o->robust_loss_width_depth_prior > 0.0))
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "robust_loss_width_depth_prior must be positive");
  }
  if (o->loss_function_type < 0 || o->loss_function_type > THEIA_LOSS_TRUNCATED)
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "invalid loss function type");  // reference: LOG(FATAL)
  return 0;
}

void fill_devproblem(theia_ba_handle_s* h) {
  h->camrot_valid = false;   // whoever rebuilds the device view may have touched cam[] / the scales: the next linearisation runs k_cam_prep
  DevProblem& P = h->P;
  P.nc = h->nc; P.np = h->np; P.ncv = h->ncv; P.ntiles = h->ntiles_main; P.nobs = h->nobs_main;
  P.n = h->n; P.pd = h->pd; P.loss_type = h->opt.loss_function_type; P.loss_width = h->opt.robust_loss_width;
  P.intr = h->intr[h->cur].p; P.intr_cand = h->intr[1 - h->cur].p;
  P.group_model = h->group_model.p; P.cam_group = h->cam_group.p;
  P.ni = h->ni; P.ng_total = h->ng; P.grp_red = h->d_grp_red.p; P.grp_free = h->d_grp_free.p; P.grp_k = h->d_grp_k.p;
  P.red_free = h->d_red_free.p; P.intr_rows = h->intr_rows;
  P.scale_i = h->scale_i.p; P.scale_red = h->scale_red.p;
  P.cam_red = h->d_cam_red.p; P.cam_mask = h->d_cam_mask.p; P.pt_const = h->d_pt_const.p;
  P.obs_uv = h->obs_uv.p; P.obs_si = h->obs_si.p; P.obs_cam = h->obs_cam.p; P.obs_pt = h->obs_pt.p;
  P.obs_kind = h->obs_kind.n ? h->obs_kind.p : nullptr; P.loss_width_depth = h->opt.robust_loss_width_depth_prior;
  P.tile_start = h->tile_start.p; P.tile_count = h->tile_count.p;
  P.scale_c = h->scale_c.p; P.scale_p = h->scale_p.p;
  P.long_nobs = h->long_nobs; P.long_ntracks = h->long_ntracks;
  P.long_obs_index = h->long_obs_index.p; P.long_obs_slot = h->long_obs_slot.p;
  P.long_track_start = h->long_track_start.p; P.long_track_pt = h->long_track_pt.p;
  P.n_priors = h->n_priors; P.prior_cam = h->prior_cam.p; P.prior_kind = h->prior_kind.p;
  P.prior_vec = h->prior_vec.p; P.prior_info = h->prior_info.p;
  P.rec = h->rec.p; P.n_diag_items = h->n_diag_items; P.n_blk_items = h->n_blk_items;
  P.n_fruns = h->use_fused ? h->n_fruns : 0; P.fruns = h->fruns.p; P.frun_order = h->frun_order.p; P.frun_next = h->frun_next.p; P.frun_cams = h->frun_cams.p; P.frun_stage = h->frun_stage.p; P.frun_tgt = h->frun_tgt.p;
  P.obs_lc = h->obs_lc.p; P.obs_tl = h->obs_tl.p; P.tile_trk_end = h->tile_trk_end.p; P.fpart = h->fpart.p; P.camrot = h->camrot.p; P.camrot_cand = h->camrot_cand.p; P.camdir = h->camdir.p;
  { const char* dbg = getenv("THEIA_HIP_FUSED_DBG"); P.fused_dbg = dbg ? atoi(dbg) : 0; }
  P.model_mask = h->model_mask;
  P.lm_cur = nullptr; P.pts_alt = nullptr;   // (set by run() around the bodies of the folded chain only)
  P.n_sum_items = h->n_sum_items; P.sum_items = h->sum_items.p; P.sum_src = h->sum_src.p;
  P.fused_bw = h->use_fused ? h->fused_bw : 0; P.n_sum_items2 = h->n_sum_items2; P.fused_kmask = h->fused_kmask;
  P.diag_items = h->diag_items.p; P.rec_slot = h->cam_obs.p; P.slot_obs = h->slot_obs.p; P.slot_pt = h->slot_pt.p; P.blk_items = h->blk_items.p; P.blk_pairs = h->blk_pairs.p;
  P.pt_sum_slot = h->n_trk_sums ? h->pt_sum_slot.p : nullptr; P.slot_in_sum = h->n_trk_sums ? h->slot_in_sum.p : nullptr;
  P.pt_sum_cnt = h->n_trk_sums ? h->pt_sum_cnt.p : nullptr; P.sum_group = h->n_trk_sums ? h->sum_group.p : nullptr; P.sum_base = h->sum_base;
}

// create()'s staged uploads sit in pinned blocks of the handle's arena until the stream is known to have passed them: every
// entry point lets them go as soon as the stream is idle (a handle used only for evaluation, covariances or reset never
// reaches the end of a run(), which is where they were released before)
void release_stage_if_idle(theia_ba_handle_s* h) {
  if (h->stage.blocks.empty()) return;
  if (hipStreamQuery(h->stream) == hipSuccess) h->stage.release();
  else (void)hipGetLastError();   // hipErrorNotReady: still copying
}

int upload_parameters(theia_ba_handle_s* h, const theia_ba_problem* p) {
  // Inside create() (a staging arena on this stream): the caller's arrays are copied into pinned blocks on host threads and
  // uploaded from there, nothing waits.  Otherwise (reset_parameters): pageable sources, the stream is waited for.
  StageArena* a = stage_arena();
  const bool staged = a && a->stream == h->stream;
  bool must_wait = false;
  auto up = [&](double* dst0, double* dst1, const double* src, size_t count) -> int {
    if (!count) return 0;
    const double* from = src;
    // (staged up to 64 MB per array -- C4's points are 16 MB; larger arrays go from the caller's memory and are waited for,
    // like PoolBuf::upload's cap: pinned blocks count against the 2 GiB pinned cache until the arena is released)
    const bool fits = count * sizeof(double) <= ((size_t)64 << 20);
    double* st = (staged && fits) ? static_cast<double*>(a->reserve(count * sizeof(double))) : nullptr;
    if (st) {
      host_chunks((int64_t)count, [&](int64_t i0, int64_t i1) { std::memcpy(st + i0, src + i0, sizeof(double) * (size_t)(i1 - i0)); });
      from = st;
    } else {
      if (staged && fits) (void)hipGetLastError();   // the host does not pin that much: the caller's array is the source, and is waited for
      must_wait = true;
    }
    HIP_TRYR(hipMemcpyAsync(dst0, from, sizeof(double) * count, hipMemcpyHostToDevice, h->stream));
    HIP_TRYR(hipMemcpyAsync(dst1, dst0, sizeof(double) * count, hipMemcpyDeviceToDevice, h->stream));
    return 0;
  };
  int rc;
  if ((rc = up(h->cam[0].p, h->cam[1].p, p->cam_ext, (size_t)6 * h->nc))) return rc;
  if ((rc = up(h->pts[0].p, h->pts[1].p, p->points, (size_t)4 * h->np))) return rc;
  if (h->ng) {
    std::vector<double> hk(p->intrinsics, p->intrinsics + (size_t)THEIA_MAX_INTRINSICS * h->ng);
    for (int g = 0; g < h->ng; ++g) if (h->grp_red[g] >= 0) project_intrinsics_to_bounds(p->group_model[g], &hk[(size_t)g * THEIA_MAX_INTRINSICS]);
    if ((rc = up(h->intr[0].p, h->intr[1].p, hk.data(), hk.size()))) return rc;
    if (must_wait) HIP_TRYR(hipStreamSynchronize(h->stream));   // (hk is a local)
  }
  if (must_wait) HIP_TRYR(hipStreamSynchronize(h->stream));
  h->cur = 0;
  h->P.intr = h->intr[0].p; h->P.intr_cand = h->intr[1].p;
  h->have_scale = false; h->camrot_valid = false;
  return 0;
}

int do_allreduce(theia_ba_handle_s* h, double* buf, size_t count, int op) {
  if (!h->allreduce || count == 0) return 0;
  const int rc = h->allreduce(h->allreduce_ctx, buf, count, op, (void*)h->stream);
  if (rc) return set_error(THEIA_HIP_ERR_INTERNAL, "allreduce callback failed (%d)", rc);
  return 0;
}

// cost of a tile range at given parameters (deterministic reduction)
int cost_of_tiles(theia_ba_handle_s* h, int tile0, int ntiles, const double* cam, const double* pts, double* cost, double* invalid) {
  *cost = 0.0; *invalid = 0.0;
  if (ntiles == 0) return 0;
  DevProblem Q = h->P;
  Q.tile_start = h->tile_start.p + tile0; Q.tile_count = h->tile_count.p + tile0; Q.ntiles = ntiles;
  HIP_TRYR(hipMemsetAsync(h->scalB.p, 0, sizeof(double) * 16, h->stream));
  launch_cost_only(Q, cam, pts, h->tile_part.p, h->scalB.p, h->stream);
  launch_reduce_tiles(ntiles, h->tile_part.p, 2, h->f2s.p + 16, h->fmaxflag.p + 16, h->scalB.p, h->stream);
  HIP_TRYR(hipMemcpyAsync(h->h_scal + 16, h->scalB.p, sizeof(double) * 16, hipMemcpyDeviceToHost, h->stream));
  HIP_TRYR(hipStreamSynchronize(h->stream));
  *cost = h->h_scal[16 + SB_COST]; *invalid = h->h_scal[16 + SB_INVALID];
  return 0;
}

// Jacobi scaling 1/(1+sqrt(colnorm^2)) from the unscaled Jacobian at the
// current point (ceres trust_region_minimizer.cc, computed once per solve).
// With several ranks the camera column norms are summed first: cameras are
// shared by all track shards.
int compute_scale(theia_ba_handle_s* h) {
  DevProblem Q = h->P;
  Q.scale_c = h->ones_c.p; Q.scale_p = h->ones_p.p;
  if (h->colsq_c0.n) HIP_TRYR(hipMemsetAsync(h->colsq_c0.p, 0, sizeof(double) * h->colsq_c0.n, h->stream));
  if (h->colsq_p0.n) HIP_TRYR(hipMemsetAsync(h->colsq_p0.p, 0, sizeof(double) * h->colsq_p0.n, h->stream));
  if (h->colsq_i0.n) HIP_TRYR(hipMemsetAsync(h->colsq_i0.p, 0, sizeof(double) * h->colsq_i0.n, h->stream));
  Q.scale_i = h->ones_i.p;
  Q.intr = h->intr[h->cur].p;
  launch_colnorm(Q, h->cam[h->cur].p, h->pts[h->cur].p, h->colsq_c0.p, h->colsq_p0.p, h->colsq_i0.p, h->stream);
  if (Q.fused_bw > 0 && Q.n_fruns > 0) {
    // camera and intrinsics columns: one pass of the fused kernel over unit scales -- its per-(camera, row) lanes already
    // sum the squared column norms, k_sum_items leaves them by reduced index, the group columns summed over the group's
    // cameras (fixed order, no atomics).  The reduced system it writes on the way is cleared by the first linearisation.
    Q.fused_dbg |= 8;   // (no pair products in this pass)
    launch_linearize_fused_intr(Q, h->cam[h->cur].p, h->pts[h->cur].p, h->ones_c.p /* radius 1 */, h->rb, h->Vinv.p, h->tile_part.p, h->stream);
    launch_scatter_colsq(Q, h->rb.colsq, h->colsq_c0.p, h->colsq_i0.p, h->stream);
  }
  launch_long_colnorm(Q, h->cam[h->cur].p, h->pts[h->cur].p, h->colsq_c0.p, h->colsq_p0.p, h->long_scratch.p, h->stream, h->colsq_i0.p);
  launch_cam_priors(Q, PRIOR_COLNORM, h->cam[h->cur].p, nullptr, nullptr, nullptr, h->colsq_c0.p, nullptr, nullptr, h->stream);
  int rc = do_allreduce(h, h->colsq_c0.p, h->colsq_c0.n, THEIA_REDUCE_SUM);
  if (!rc && h->ni) rc = do_allreduce(h, h->colsq_i0.p, h->colsq_i0.n, THEIA_REDUCE_SUM);
  if (rc) return rc;
  launch_make_scale((int)h->colsq_c0.n, h->colsq_c0.p, h->scale_c.p, h->stream);
  launch_make_scale((int)h->colsq_p0.n, h->colsq_p0.p, h->scale_p.p, h->stream);
  launch_make_scale((int)h->colsq_i0.n, h->colsq_i0.p, h->scale_i.p, h->stream);
  launch_build_scale_red(h->P, h->scale_red.p, h->stream);
  h->have_scale = true; h->camrot_valid = false;   // (the blocks carry the Jacobi scaling of the extrinsics columns)
  return 0;
}

// Where the Jacobi scaling is folded into the first linearisation of a run (enqueue_linearize(.., first_fold = true)) instead
// of taking compute_scale()'s pass of its own.  The fold applies to: the fused plan without free intrinsics (k_lin_schur),
// on one rank (the norms need no all-reduce), with every track inside a wave tile (no slow-path tracks), without camera
// priors (their rows add to the column norms after the launch), with a reduced system to rescale, and with direct launches
// (the opt-in graph replay would capture the first body as the replayed one).  Inner iterations take the fold too.
// Everything else keeps the separate pass; THEIA_HIP_SCALE_PASS=1 forces it.
bool scale_fold_applies(const theia_ba_handle_s* h) {
  const char* pass = getenv("THEIA_HIP_SCALE_PASS");
  const char* genv = getenv("THEIA_HIP_LM_GRAPH");
  return h->use_fused && h->ni == 0 && h->n_fruns > 0 && h->n_sum_items > 0 && h->n > 0 && h->ntiles_main > 0 && !h->allreduce &&
         h->long_ntracks == 0 && h->n_priors == 0 && !(genv && genv[0] == '1') && !(pass && pass[0] == '1');
}

// Where run() takes the folded LM chain for its bodies: per iteration
//   k_lin_schur -> k_schur_sum<glue> -> K3 levels -> k_cam_update<1> (+ the linearisation's scalars, + clear of S) ->
//   k_backsub_runs -> k_reduce_tiles_stage1 -> k_reduce_control (+ clear of the scalars) -> the next k_lin_schur
// instead of the chain with k_sp_clear, the linearisation's k_reduce_tiles_stage1, k_finalize_rcs, k_sp_symm and k_lm_accept
// in launches of their own.  An accepted step flips LmState::cur instead of copying the candidate over the
// state: the three kernels that read parameters select their buffers by it (DevProblem::lm_cur), and run() swaps the
// handle's own pointers after its last read-back if the state ended in the second buffers.  The first body of a run keeps
// the glue launches but k_lm_accept (nothing assumes a clean S on entry, and with the scale fold k_sp_rescale stands
// between the sums and the LM diagonal); it already clears behind itself.
// It applies to: the fused plan without free intrinsics, on one rank, every track inside a wave tile, no camera priors,
// direct launches, a sparse K3 plan, every row of the system owned by a camera that k_schur_sum visits, and the candidate's
// blocks written by k_cam_update's extra workgroups, k_backsub_runs for the trial step, a handle without inner-iteration
// lists.  run() adds: no phase timing.
// THEIA_HIP_LM_GLUE_KERNELS=1 keeps the separate launches everywhere (A/B runs, the equality test).
bool lm_glue_applies(const theia_ba_handle_s* h) {
  const char* keep = getenv("THEIA_HIP_LM_GLUE_KERNELS");
  const char* genv = getenv("THEIA_HIP_LM_GRAPH");
  if ((keep && keep[0] == '1') || (genv && genv[0] == '1')) return false;
  if (!(h->use_fused && h->ni == 0 && h->n_fruns > 0 && h->n_sum_items > 0 && h->n > 0 && h->ntiles_main > 0 && !h->allreduce &&
        !h->dist_k3 && h->long_ntracks == 0 && h->n_priors == 0 && h->sum_covers_n))
    return false;
  // (the state's per-camera blocks stay current between bodies -- enqueue_linearize: keep_blocks -- so no k_cam_prep, which
  // does not look at LmState::cur, runs after the first body)
  if (h->inner || getenv("THEIA_HIP_CAM_PREP_ALWAYS")) return false;
  return cam_update_preps(h->P) == 1 && backsub_runs_applies(h->P) && linearize_route(h->P) == LIN_FUSED &&
         chol_plan_tile_lists(h->plan).nzero > 0;
}

// what run() branches on: the chain applies to the handle, and this run has no inner iterations, no phase timing
bool lm_glue_run(const theia_ba_handle_s* h) {
  const bool inner = h->inner && h->opt.use_inner_iterations != 0;
  return lm_glue_applies(h) && !inner && getenv("THEIA_HIP_PHASE_TIMING") == nullptr;
}

// enqueue: clear, linearize + Schur, tile reduction, (all-reduce), LM diagonal.
// The trust-region radius is read from the device-resident LM state.
// slot < 0: no phase-timing events (graph capture, or timing not requested)
// first_fold: the first linearisation of a run where scale_fold_applies(): it also makes the Jacobi scaling
// chain == LM_FOLDED: a later body of a run on the folded chain (lm_glue_applies): no clear, k_schur_sum finishes the system
int enqueue_linearize(theia_ba_handle_s* h, int slot, bool first_fold, LmChain chain) {
  const bool folded = chain == LM_FOLDED;
  const double* radius = &reinterpret_cast<const LmState*>(h->lm_state.p)->radius;
  h->P.intr = h->intr[h->cur].p; h->P.intr_cand = h->intr[1 - h->cur].p;
  // clear the reduced system: the tiles the K3 plan knows (assembly + fill) and the vector tail; everything else in
  // the n x n buffer is never written (it was zeroed once at create())
  const bool plan_clears = !folded && h->n > 0 && !(h->allreduce && h->n_pack_tiles == 0) &&
                           chol_plan_clear(h->plan, h->rb.S, h->n, h->stream, h->rb.rhs, h->reduce.n - (size_t)h->n * h->n);
  if (!folded && !plan_clears) HIP_TRYR(hipMemsetAsync(h->reduce.p, 0, sizeof(double) * h->reduce.n, h->stream));
  if (slot >= 0) HIP_TRYR(hipEventRecord(h->ev[slot][4], h->stream));
  // the state's per-camera blocks (k_cam_prep) are still current after the first body: an accepted step copies the candidate's
  // blocks over them (k_lm_accept), a rejected one leaves the state where it was.  Not with inner iterations (the accepted
  // point may be the swept one, and the sweep reuses the candidate's blocks) and not with free intrinsics.
  const bool keep_blocks = h->use_fused && h->ni == 0 && !h->inner && !getenv("THEIA_HIP_CAM_PREP_ALWAYS");
  h->P.camrot_current = keep_blocks && h->camrot_valid;
  if (folded) {
    // the body before this one left the plan's tiles and the scalars clear; k_schur_sum finishes the system, the scalars of
    // the linearisation wait in tile_part / red_part for k_cam_update's folding workgroup (the trial step reuses both later)
    const CholTileLists tl = chol_plan_tile_lists(h->plan);
    const bool two_stage = h->ntiles_main > 4 * kReduceBlocks;
    const LinGlue lg{h->scale_red.p, tl.symm_map, tl.nt, h->fmaxflag.p, two_stage ? h->red_part.p : nullptr};
    launch_linearize_fused(h->P, h->cam[h->cur].p, h->pts[h->cur].p, radius, h->rb, h->Vinv.p, h->tile_part.p, h->stream, &lg);
    h->camrot_valid = keep_blocks;
    return 0;
  }
  if (first_fold) {
    // unit scales in, scale_p / scale_c / scale_red out; the camera scaling factors out of the Schur complement exactly
    // (S(D) = D S(I) D, rhs(D) = D rhs(I), the same for g_c and the column norms), so the assembled system is rescaled
    // before the LM diagonal, and the state's per-camera blocks are rebuilt with the solve's scales for the back-substitution
    launch_linearize_fused_first(h->P, h->ones_c.p, h->ones_p.p, h->scale_c.p, h->scale_p.p, h->scale_red.p, h->cam[h->cur].p,
                                 h->pts[h->cur].p, radius, h->rb, h->Vinv.p, h->tile_part.p, h->stream);
    chol_plan_rescale(h->plan, h->rb.S, h->n, h->n, h->scale_red.p, h->rb.rhs, h->rb.colsq, h->rb.gc, h->stream);
    launch_cam_prep(h->P, h->cam[h->cur].p, h->P.intr, h->P.camrot, h->stream);
    h->have_scale = true;
  } else
  launch_linearize(h->P, h->cam[h->cur].p, h->pts[h->cur].p, radius, h->rb, h->Vinv.p, h->gp.p, h->tile_part.p, h->stream);
  h->camrot_valid = keep_blocks;
  if (slot >= 0) HIP_TRYR(hipEventRecord(h->ev[slot][5], h->stream));
  // without an all-reduce (and without phase timing) the tile reduction rides in k_finalize_rcs: one launch less
  const bool fuse_reduce = !h->allreduce && slot < 0 && h->ntiles_main > 0;
  if (h->ntiles_main && !fuse_reduce) launch_reduce_tiles(h->ntiles_main, h->tile_part.p, 4, h->f2s.p, h->fmaxflag.p, h->rb.scal, h->stream, h->red_part.p);
  launch_long_linearize(h->P, h->cam[h->cur].p, h->pts[h->cur].p, radius, h->rb, h->Vinv.p, h->gp.p, h->long_scratch.p, h->stream);
  launch_cam_priors(h->P, PRIOR_LINEARIZE, h->cam[h->cur].p, nullptr, nullptr, &h->rb, nullptr, h->rb.scal + SC_COST, nullptr, h->stream);
  // one SUM all-reduce of [S | rhs | colsq | gc | scal[0,8)], one MAX of scal[8,16) (folded into the SUM as
  // per-rank slots when the shard geometry is known)
  int rc = 0;
  bool max_done = false;
  if (h->dist_k3) {
    // the rank's private columns: LM diagonal, then their factorisation from this rank's sums alone (their Schur
    // complement lands in the shared tiles and the shared rows of the rhs, which the all-reduce sums next)
    launch_finalize_rcs(h->P, radius, h->rb, h->stream, 0, nullptr, nullptr, nullptr, h->d_tile_cls.p, 1);
    chol_plan_solve_phase(h->plan, 0, h->rb.S, h->n, h->rb.rhs, h->chol_work.p, h->rb.scal + SC_NOTPD, h->stream);
  }
  if (h->allreduce && h->n_pack_tiles > 0 && h->n > 0) {
    const int tail_blocks = (int)((3 * (size_t)h->n + 8 + 255) / 256);
    const int grid = h->n_pack_tiles + std::max(1, std::min(tail_blocks, 64));
    const int world = (h->shard_world > 0 && h->shard_rank >= 0 && h->shard_rank < h->shard_world && h->shard_world <= kMaxShardSlots)
                          ? h->shard_world : 0;
    k_pack_rcs<<<grid, 256, 0, h->stream>>>(h->n, h->reduce.p, h->pack_tiles.p, h->n_pack_tiles, h->pack_buf.p, 1, h->shard_rank, world);
    rc = do_allreduce(h, h->pack_buf.p, (size_t)h->n_pack_tiles * 4096 + 3 * (size_t)h->n + 8 + world, THEIA_REDUCE_SUM);
    k_pack_rcs<<<grid, 256, 0, h->stream>>>(h->n, h->reduce.p, h->pack_tiles.p, h->n_pack_tiles, h->pack_buf.p, 0, h->shard_rank, world);
    max_done = world > 0;
  } else {
    rc = do_allreduce(h, h->reduce.p, (size_t)h->n * h->n + 3 * (size_t)h->n + 8, THEIA_REDUCE_SUM);
  }
  if (!rc && !max_done) rc = do_allreduce(h, h->rb.scal + 8, 8, THEIA_REDUCE_MAX);
  if (rc) return rc;
  if (fuse_reduce && h->ntiles_main > 4 * kReduceBlocks) {   // two stages: one workgroup over 50k tile rows costs 45 us
    launch_reduce_tiles_stage1(h->ntiles_main, h->tile_part.p, 4, h->fmaxflag.p, h->red_part.p, h->stream);
    launch_finalize_rcs(h->P, radius, h->rb, h->stream, kReduceBlocks, h->red_part.p, h->f2s.p, h->fmaxflag.p);
  } else if (fuse_reduce) launch_finalize_rcs(h->P, radius, h->rb, h->stream, h->ntiles_main, h->tile_part.p, h->f2s.p, h->fmaxflag.p);
  else if (h->dist_k3) launch_finalize_rcs(h->P, radius, h->rb, h->stream, 0, nullptr, nullptr, nullptr, h->d_tile_cls.p, 0);   // the shared columns
  else launch_finalize_rcs(h->P, radius, h->rb, h->stream);
  return 0;
}

// enqueue: dense solve, candidate cameras, back-substitution + trial cost.
// defer_reduce: the tile reduction of the trial step is left to k_reduce_control (no all-reduce in between).
int enqueue_solve_and_backsub(theia_ba_handle_s* h, int slot, bool defer_reduce, LmChain chain) {
  double* yc = h->rb.rhs;  // the solution overwrites the rhs row
  // (folded: k_schur_sum has written the mirrored tiles; phase 0 of an unsharded plan is nothing but k_sp_symm)
  if (chain == LM_FOLDED) chol_plan_solve_phase(h->plan, 1, h->rb.S, h->n, h->rb.rhs, h->chol_work.p, h->rb.scal + SC_NOTPD, h->stream);
  else if (h->dist_k3) {
    chol_plan_solve_phase(h->plan, 1, h->rb.S, h->n, h->rb.rhs, h->chol_work.p, h->rb.scal + SC_NOTPD, h->stream);
    k_y_own<<<(h->n + 255) / 256, 256, 0, h->stream>>>(h->n, yc, h->d_tile_cls.p, h->shard_rank);
    const int rcy = do_allreduce(h, yc, (size_t)h->n, THEIA_REDUCE_SUM);
    if (rcy) return rcy;
  } else
  chol_plan_solve(h->plan, h->rb.S, h->n, h->rb.rhs, h->chol_work.p, h->rb.scal + SC_NOTPD, h->stream);
  if (slot >= 0) HIP_TRYR(hipEventRecord(h->ev[slot][2], h->stream));
  const int nxt = 1 - h->cur;
  // LM_FOLD_FIRST, LM_FOLDED: S is dead once the solve has left y in the row behind it (h->rb.rhs = S + n * n, outside every tile of the plan):
  // the tiles the next body's assembly and factorisation touch are cleared beside the candidate cameras; LM_FOLDED: the
  // scalars of the linearisation (k_schur_sum's stage-1 sums, or the per-tile partials) are folded into rb.scal there too
  CamUpdateGlue cg{};
  if (chain != LM_SEPARATE) {
    const CholTileLists tl = chol_plan_tile_lists(h->plan);
    cg.zero_S = h->rb.S; cg.zero_items = tl.zero_items; cg.nzero = tl.nzero;
  }
  if (chain == LM_FOLDED) {
    const bool two_stage = h->ntiles_main > 4 * kReduceBlocks;
    cg.lin_part = two_stage ? h->red_part.p : h->tile_part.p; cg.lin_ntiles = two_stage ? kReduceBlocks : h->ntiles_main;
    cg.lin_f2s = h->f2s.p; cg.lin_fmaxflag = h->fmaxflag.p; cg.scal = h->rb.scal;
  }
  launch_cam_update(h->P, h->cam[h->cur].p, yc, h->cam[nxt].p, h->ni ? h->intr[nxt].p : nullptr,
                    h->scalB.p + SB_STEPSQ_CAM, h->scalB.p + SB_XNORMSQ_CAM, h->stream, h->scalB.p, chain != LM_SEPARATE ? &cg : nullptr);
  launch_backsub(h->P, h->cam[h->cur].p, h->pts[h->cur].p, h->cam[nxt].p, h->pts[nxt].p, yc, h->Vinv.p, h->tile_part.p, h->scalB.p, h->stream);
  if (h->ntiles_main && !defer_reduce) launch_reduce_tiles(h->ntiles_main, h->tile_part.p, 5, h->f2s.p + 8, h->fmaxflag.p + 8, h->scalB.p, h->stream, h->red_part.p);
  launch_long_backsub(h->P, h->cam[h->cur].p, h->pts[h->cur].p, h->cam[nxt].p, h->pts[nxt].p, yc, h->Vinv.p, h->long_scratch.p, h->scalB.p, h->stream);
  launch_cam_priors(h->P, PRIOR_TRIAL, h->cam[h->cur].p, h->cam[nxt].p, yc, nullptr, nullptr, h->scalB.p + SB_COST, h->scalB.p + SB_MCC, h->stream);
  return do_allreduce(h, h->scalB.p, 8, THEIA_REDUCE_SUM);
}

// The all-reduced S has the union of the ranks' tile structures: OR the tile
// co-visibility over the ranks (MAX all-reduce) and rebuild the K3 schedule.
int sync_plan(theia_ba_handle_s* h) {
  const int nt = (h->n + 63) / 64;
  const size_t cnt = (size_t)nt * nt;
  h->dist_k3 = false;
  if (cnt == 0 || !h->allreduce) { h->plan_is_global = true; return 0; }
  if (h->tile_adj_local.size() != cnt) h->tile_adj_local = h->tile_adj;   // this rank's own structure (tile_adj becomes the union)
  std::vector<double> a(cnt);
  for (size_t i = 0; i < cnt; ++i) a[i] = h->tile_adj_local[i];
  HIP_TRYR(hipMemcpyAsync(h->reduce.p, a.data(), sizeof(double) * cnt, hipMemcpyHostToDevice, h->stream));
  int rc = do_allreduce(h, h->reduce.p, cnt, THEIA_REDUCE_MAX);
  if (rc) return rc;
  HIP_TRYR(hipMemcpyAsync(a.data(), h->reduce.p, sizeof(double) * cnt, hipMemcpyDeviceToHost, h->stream));
  HIP_TRYR(hipStreamSynchronize(h->stream));
  for (size_t i = 0; i < cnt; ++i) h->tile_adj[i] = a[i] != 0.0 ? 1 : 0;
  h->drop_graph();
  if (h->plan) chol_plan_destroy(h->plan);
  h->plan = nullptr;
  // Distributed K3 (round 4): with the shard geometry declared (set_shard / set_rccl), no intrinsics columns and more than one
  // rank, a tile column that only ONE rank's tracks touch is factored by that rank alone, before the all-reduce, which then
  // carries the shared tiles only.  Every rank takes the same decision from the same all-reduced numbers.
  const bool geom = h->shard_world > 1 && h->shard_rank >= 0 && h->shard_rank < h->shard_world && h->shard_world <= kMaxShardSlots;
  if (geom && h->ni == 0 && nt > 2 && !getenv("THEIA_HIP_K3_REPLICATED")) {
    std::vector<double> t(nt + 1, 0.0);
    for (int i = 0; i < nt; ++i) t[i] = (i < (int)h->tile_touch.size() && h->tile_touch[i]) ? 1.0 : 0.0;
    HIP_TRYR(hipMemcpyAsync(h->reduce.p, t.data(), sizeof(double) * nt, hipMemcpyHostToDevice, h->stream));
    if ((rc = do_allreduce(h, h->reduce.p, (size_t)nt, THEIA_REDUCE_SUM))) return rc;
    std::vector<double> c(nt);
    HIP_TRYR(hipMemcpyAsync(c.data(), h->reduce.p, sizeof(double) * nt, hipMemcpyDeviceToHost, h->stream));
    HIP_TRYR(hipStreamSynchronize(h->stream));
    h->tile_cls.assign(nt, 0);
    int nmine = 0;
    for (int i = 0; i < nt; ++i)
      if (c[i] == 1.0) { h->tile_cls[i] = t[i] != 0.0 ? 1 : 2; nmine += t[i] != 0.0; }
    CholPlan* pl = chol_plan_create_sharded(h->n, h->tile_adj.data(), h->tile_cls.data());
    double bad = pl ? 0.0 : 1.0;      // agreed between the ranks: one rank without a level schedule keeps everybody replicated
    HIP_TRYR(hipMemcpyAsync(h->reduce.p, &bad, sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRYR(hipStreamSynchronize(h->stream));
    if ((rc = do_allreduce(h, h->reduce.p, 1, THEIA_REDUCE_MAX))) { if (pl) chol_plan_destroy(pl); return rc; }
    HIP_TRYR(hipMemcpyAsync(&bad, h->reduce.p, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRYR(hipStreamSynchronize(h->stream));
    if (bad == 0.0) {
      h->plan = pl; h->dist_k3 = true;
      if ((rc = h->d_tile_cls.upload(h->tile_cls, h->stream))) return rc;
      if (getenv("THEIA_HIP_CREATE_TIMING"))
        fprintf(stderr, "theia_hip distributed K3: rank %d of %d, %d of %d tiles private, %d levels before the all-reduce, %zu shared tiles in it\n",
                h->shard_rank, h->shard_world, nmine, nt, chol_plan_split_level(pl), chol_plan_shared_tiles(pl).size() / 2);
    } else {
      if (getenv("THEIA_HIP_CREATE_TIMING"))
        fprintf(stderr, "theia_hip distributed K3: rank %d of %d keeps the replicated plan (%d of %d tiles private here; %s)\n", h->shard_rank,
                h->shard_world, nmine, nt, pl ? "another rank has no level schedule" : "no level schedule for this rank's structure");
      if (pl) chol_plan_destroy(pl);
    }
  } else if (getenv("THEIA_HIP_CREATE_TIMING") && h->shard_world > 1)
    fprintf(stderr, "theia_hip distributed K3: not taken (shard geometry %d/%d, %d intrinsics columns, %d tiles)\n", h->shard_rank, h->shard_world, h->ni, nt);
  if (!h->plan) h->plan = chol_plan_create(h->n, h->tile_adj.data());
  h->plan_is_global = true;
  HIP_TRYR(hipMemsetAsync(h->reduce.p, 0, sizeof(double) * h->reduce.n, h->stream));   // tiles only the old plan touched
  {
    std::vector<int2> tiles;
    if (h->dist_k3) {
      const std::vector<int>& st = chol_plan_shared_tiles(h->plan);
      for (size_t k = 0; k + 1 < st.size(); k += 2) tiles.push_back(make_int2(st[k], st[k + 1]));
      if (tiles.empty()) tiles.push_back(make_int2(0, 0));   // (the packed path needs one)
    } else
    for (int i = 0; i < nt; ++i)
      for (int j = 0; j <= i; ++j)
        if (i == j || h->tile_adj[(size_t)i * nt + j]) tiles.push_back(make_int2(i, j));
    h->n_pack_tiles = (int)tiles.size();
    int rc2 = h->pack_tiles.upload(tiles, h->stream);
    if (!rc2) rc2 = h->pack_buf.alloc((size_t)tiles.size() * 4096 + 3 * (size_t)h->n + 8 + kMaxShardSlots);
    if (rc2) return rc2;
    HIP_TRYR(hipStreamSynchronize(h->stream));
  }
  return 0;
}

// An error left behind by an earlier, deliberately ignored HIP call of this host thread (a refused cooperative launch, an
// event of a destroyed stream, another library) must not be mistaken for a failure of THIS call: run() asks hipGetLastError()
// after it has enqueued its kernels.  The entry points therefore start from a clean slate; THEIA_HIP_DEBUG_STICKY=1 reports
// what was discarded (one box in six showed a stale "operation not permitted when stream is capturing" here, origin unknown).
void debug_sticky(const char* where) {
  static const bool report = getenv("THEIA_HIP_DEBUG_STICKY") != nullptr;
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess && report) std::fprintf(stderr, "theia_hip: stale HIP error discarded at %s: %s\n", where, hipGetErrorString(e));
}

}  // namespace thip

extern "C" {

void theia_ba_options_default(theia_ba_options* o) {
  std::memset(o, 0, sizeof(*o));
  o->loss_function_type = THEIA_LOSS_TRIVIAL;
  o->robust_loss_width = 2.0;
  o->intrinsics_to_optimize = THEIA_INTR_NONE;
  o->max_num_iterations = 100;
  o->use_homogeneous_point_parametrization = 1;
  o->use_inner_iterations = 1;
  o->function_tolerance = 1e-6;
  o->gradient_tolerance = 1e-10;
  o->parameter_tolerance = 1e-8;
  o->max_trust_region_radius = 1e12;
  o->max_solver_time_in_seconds = 3600.0;
  o->robust_loss_width_depth_prior = 0.01;   // bundle_adjustment.h:94
}

int theia_hip_ba_reset_parameters(theia_ba_handle h, const theia_ba_problem* p) {
  if (!h || !p) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (h->idh) return thip::id_handle_reset(h->idh, p);
  if (p->num_cameras != h->nc || p->num_points != h->np || p->num_groups != h->ng)
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "problem shape differs from the handle's");
  release_stage_if_idle(h);
  return upload_parameters(h, p);
}

int theia_hip_ba_set_shard(theia_ba_handle h, int32_t rank, int32_t world_size) {
  if (!h) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null handle");
  if (world_size < 1 || rank < 0 || rank >= world_size) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "rank / world_size out of range");
  h->shard_rank = rank; h->shard_world = world_size;
  h->have_scale = false; h->camrot_valid = false;   // the Jacobi scales are all-reduced over the new geometry: recomputed, and the camera blocks with them
  return 0;
}

int theia_hip_ba_snapshot_parameters(theia_ba_handle h) {
  if (h && h->idh) return thip::id_handle_snapshot(h->idh);
  if (!h) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null handle");
  release_stage_if_idle(h);
  int rc;
  if ((rc = h->snap_cam.alloc(h->cam[0].n)) || (rc = h->snap_pts.alloc(h->pts[0].n)) || (rc = h->snap_intr.alloc(h->intr[0].n))) return rc;
  const int c = h->cur;
  if (h->cam[c].n) HIP_TRYR(hipMemcpyAsync(h->snap_cam.p, h->cam[c].p, sizeof(double) * h->cam[c].n, hipMemcpyDeviceToDevice, h->stream));
  if (h->pts[c].n) HIP_TRYR(hipMemcpyAsync(h->snap_pts.p, h->pts[c].p, sizeof(double) * h->pts[c].n, hipMemcpyDeviceToDevice, h->stream));
  if (h->intr[c].n) HIP_TRYR(hipMemcpyAsync(h->snap_intr.p, h->intr[c].p, sizeof(double) * h->intr[c].n, hipMemcpyDeviceToDevice, h->stream));
  h->has_snapshot = true;
  return 0;
}

int theia_hip_ba_restore_parameters(theia_ba_handle h) {
  if (h && h->idh) return thip::id_handle_restore(h->idh);
  if (!h) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null handle");
  if (!h->has_snapshot) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "no snapshot taken on this handle");
  release_stage_if_idle(h);
  for (int k = 0; k < 2; ++k) {
    if (h->cam[k].n) HIP_TRYR(hipMemcpyAsync(h->cam[k].p, h->snap_cam.p, sizeof(double) * h->cam[k].n, hipMemcpyDeviceToDevice, h->stream));
    if (h->pts[k].n) HIP_TRYR(hipMemcpyAsync(h->pts[k].p, h->snap_pts.p, sizeof(double) * h->pts[k].n, hipMemcpyDeviceToDevice, h->stream));
    if (h->intr[k].n) HIP_TRYR(hipMemcpyAsync(h->intr[k].p, h->snap_intr.p, sizeof(double) * h->intr[k].n, hipMemcpyDeviceToDevice, h->stream));
  }
  h->cur = 0;
  h->P.intr = h->intr[0].p; h->P.intr_cand = h->intr[1].p;
  h->have_scale = false; h->camrot_valid = false;
  return 0;
}

int theia_hip_ba_set_options(theia_ba_handle h, const theia_ba_options* o) {
  if (!h || !o) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (h->idh) {   // the run checks the structural options against the ones the object was created with
    if (o->intrinsics_to_optimize != h->opt.intrinsics_to_optimize || o->constant_camera_position != h->opt.constant_camera_position ||
        o->constant_camera_orientation != h->opt.constant_camera_orientation || o->prior_mask != h->opt.prior_mask)
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "structural options differ from the ones the handle was created with");
    h->opt = *o;
    return 0;
  }
  const theia_ba_options& c = h->opt;
  if (o->use_homogeneous_point_parametrization != c.use_homogeneous_point_parametrization ||
      o->constant_camera_orientation != c.constant_camera_orientation ||
      o->constant_camera_position != c.constant_camera_position || o->orthographic_camera != c.orthographic_camera ||
      o->intrinsics_to_optimize != c.intrinsics_to_optimize || o->prior_mask != c.prior_mask)
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "structural options differ from the ones the handle was created with");
  if (o->use_inner_iterations && !h->inner && h->nobs_main > 0)
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "use_inner_iterations: the handle was created without the inner-iteration lists");
  if (o->loss_function_type < 0 || o->loss_function_type > THEIA_LOSS_TRUNCATED)
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "invalid loss function type");
  if (o->loss_function_type != h->opt.loss_function_type || o->robust_loss_width != h->opt.robust_loss_width ||
      o->robust_loss_width_depth_prior != h->opt.robust_loss_width_depth_prior)
    h->drop_graph();   // the loss is baked into the captured kernel arguments
  h->opt = *o;
  h->P.loss_type = o->loss_function_type;
  h->P.loss_width = o->robust_loss_width;
  h->P.loss_width_depth = o->robust_loss_width_depth_prior;
  return 0;
}

int theia_hip_ba_set_allreduce(theia_ba_handle h, theia_allreduce_fn fn, void* ctx) {
  if (h && h->idh) return set_error(THEIA_HIP_ERR_UNSUPPORTED, "inverse-depth handle: sharding is not built in this mode");
  if (!h) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null handle");
  h->allreduce = fn; h->allreduce_ctx = ctx;
  h->plan_is_global = (fn == nullptr);   // the K3 schedule must cover every rank's tracks
  return 0;
}

int theia_hip_ba_set_inner_global(theia_ba_handle h, const theia_ba_problem* full, const int64_t* point_global_index) {
  if (!h || !full || (h->np > 0 && !point_global_index)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (h->idh) return set_error(THEIA_HIP_ERR_UNSUPPORTED, "inverse-depth handle: sharding is not built in this mode");
  if (!h->inner) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "the handle was created without use_inner_iterations");
  if (full->num_cameras != h->nc || full->num_groups != h->ng)
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "the full problem must carry the shard's cameras and intrinsics groups");
  if (full->num_obs > 0 && (!full->obs_uv || !full->obs_cam || !full->obs_pt)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null observation array");
  const int64_t nobs = full->num_obs;
  const int gnp = full->num_points;
  if (nobs >= (int64_t)1 << 31) return set_error(THEIA_HIP_ERR_UNSUPPORTED, "more than 2^31 observations");
  std::vector<int> gp(h->np);
  for (int i = 0; i < h->np; ++i) {
    if (point_global_index[i] < 0 || point_global_index[i] >= gnp) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "point_global_index out of range");
    gp[i] = (int)point_global_index[i];
  }
  for (int64_t i = 0; i < nobs; ++i)
    if (full->obs_cam[i] < 0 || full->obs_cam[i] >= h->nc || full->obs_pt[i] < 0 || full->obs_pt[i] >= gnp)
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "observation index out of range");
  hipStream_t st = h->stream;
  int rc = 0;
  // observation lists by camera and by intrinsics group (depth-prior rows do not depend on the intrinsics), in the caller's order
  std::vector<int> coff(h->nc + 1, 0), cidx(nobs), goff(h->ng + 1, 0), gidx;
  for (int64_t i = 0; i < nobs; ++i) coff[full->obs_cam[i] + 1]++;
  for (int c = 0; c < h->nc; ++c) coff[c + 1] += coff[c];
  { std::vector<int> fill(coff.begin(), coff.end() - 1); for (int64_t i = 0; i < nobs; ++i) cidx[fill[full->obs_cam[i]]++] = (int)i; }
  if (h->ni) {
    auto is_depth = [&](int64_t i) { return full->obs_kind && full->obs_kind[i]; };
    for (int64_t i = 0; i < nobs; ++i) if (!is_depth(i)) goff[full->cam_group[full->obs_cam[i]] + 1]++;
    for (int g = 0; g < h->ng; ++g) goff[g + 1] += goff[g];
    gidx.resize(goff[h->ng]);
    std::vector<int> fill(goff.begin(), goff.end() - 1);
    for (int64_t i = 0; i < nobs; ++i) if (!is_depth(i)) gidx[fill[full->cam_group[full->obs_cam[i]]]++] = (int)i;
  }
  if (gidx.empty()) gidx.push_back(0);
  std::vector<int> pc, pk;
  std::vector<double> pv, pi;
  collect_cam_priors(full, h->opt.prior_mask, h->nc, nullptr, pc, pk, pv, pi);   // the priors of ALL cameras: the shards carry them on one rank only
  h->g_npriors = (int)pc.size(); h->g_np = gnp; h->g_nobs = nobs;
  std::vector<int> oc(full->obs_cam, full->obs_cam + nobs), op(full->obs_pt, full->obs_pt + nobs);
  if ((rc = h->g_uv.upload(reinterpret_cast<const double2*>(full->obs_uv), (size_t)nobs, st, false)) ||
      (rc = h->g_cam.upload(oc, st)) || (rc = h->g_pt.upload(op, st)) || (rc = h->g_cam_off.upload(coff, st)) || (rc = h->g_cam_idx.upload(cidx, st)) ||
      (rc = h->g_grp_off.upload(goff, st)) || (rc = h->g_grp_idx.upload(gidx, st)) || (rc = h->g_pidx.upload(gp, st)) ||
      (rc = h->g_prior_cam.upload(pc, st)) || (rc = h->g_prior_kind.upload(pk, st)) || (rc = h->g_prior_vec.upload(pv, st)) ||
      (rc = h->g_prior_info.upload(pi, st)) || (rc = h->g_pts.alloc((size_t)4 * std::max(1, gnp))) || (rc = h->g_stage.alloc(8)))
    return rc;
  if (full->obs_sqrt_info) { if ((rc = h->g_si.upload(reinterpret_cast<const double2*>(full->obs_sqrt_info), (size_t)nobs, st, false))) return rc; }
  else if ((rc = h->g_si.alloc(0))) return rc;
  if (full->obs_kind) { if ((rc = h->g_kind.upload(full->obs_kind, (size_t)nobs, st, false))) return rc; }
  else if ((rc = h->g_kind.alloc(0))) return rc;
  HIP_TRYR(hipStreamSynchronize(st));   // the sources above are local vectors and the caller's arrays
  h->inner_global = true;
  return 0;
}

int theia_hip_ba_plan_info(theia_ba_handle h, int32_t* n, int32_t* k3_levels, double* k3_flops, int32_t* fused_runs,
                           int32_t* slow_path_tracks) {
  if (h && h->idh) {   // (no fused runs / slow-path tracks in this mode: the per-track kernels of ba_invdepth.hip)
    thip::id_handle_plan_info(h->idh, n, k3_levels, k3_flops);
    if (fused_runs) *fused_runs = 0;
    if (slow_path_tracks) *slow_path_tracks = 0;
    return 0;
  }
  if (!h) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null handle");
  if (n) *n = h->n;
  if (k3_levels) *k3_levels = chol_plan_levels(h->plan);
  if (k3_flops) *k3_flops = chol_plan_flops(h->plan);
  if (fused_runs) *fused_runs = h->use_fused ? h->n_fruns : 0;
  if (slow_path_tracks) *slow_path_tracks = h->long_ntracks;
  return 0;
}

int theia_hip_ba_download(theia_ba_handle h, theia_ba_problem* p) {
  if (!h || !p) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (h->idh) return thip::id_handle_download(h->idh, p);
  // caller-owned (pageable) destinations: drain the stream, then blocking copies
  HIP_TRYR(hipStreamSynchronize(h->stream));
  h->stage.release();
  if (h->nc) HIP_TRYR(hipMemcpy(p->cam_ext, h->cam[h->cur].p, sizeof(double) * 6 * h->nc, hipMemcpyDeviceToHost));
  if (h->np) HIP_TRYR(hipMemcpy(p->points, h->pts[h->cur].p, sizeof(double) * 4 * h->np, hipMemcpyDeviceToHost));
  if (h->ng && h->ni) HIP_TRYR(hipMemcpy(p->intrinsics, h->intr[h->cur].p, sizeof(double) * THEIA_MAX_INTRINSICS * h->ng, hipMemcpyDeviceToHost));
  return 0;
}

int theia_hip_ba_destroy(theia_ba_handle h) {
  debug_sticky("destroy entry");
  delete h;
  debug_sticky("destroy exit");
  return 0;
}

int theia_hip_ba_run(theia_ba_handle h, theia_ba_summary* S) {
  if (!h || !S) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (h->idh) return thip::id_handle_run(h->idh, &h->opt, S);
  debug_sticky("run entry");
  release_stage_if_idle(h);   // (a previous run() that returned early with an error did not reach its release)
  const theia_ba_options& O = h->opt;
  const double t_start = now_s();
  S->trace_size = 0; S->success = 0; S->num_iterations = 0; S->num_successful_steps = 0;
  S->time_linearize = S->time_solve_reduced = S->time_backsub = 0.0;
  S->time_kernel_linearize = 0.0; S->num_linearize_launches = 0;
  S->setup_time_in_seconds = 0.0;
  int rc = h->plan_is_global ? 0 : sync_plan(h);
  if (rc) return rc;
  h->cur = 0;   // state = buffer 0, candidate = buffer 1 (accepted steps are copied back on the device)
  const bool fold = scale_fold_applies(h);   // the first body makes the Jacobi scaling itself
  if (!fold && (rc = compute_scale(h))) return rc;
  // device-resident LM state, control block and trace
  LmState st;
  std::memset(&st, 0, sizeof(st));
  lm::start(st); st.first = 1;
  st.term = THEIA_TERM_NO_CONVERGENCE; st.pending_grad = -1;
  // inner iterations need every residual block of a camera on this rank: a sharded solve that asks for them (the
  // reference's default, bundle_adjustment.h:144) is refused instead of silently walking another trajectory
  if (h->allreduce && O.use_inner_iterations != 0 && h->nobs > 0 && !h->inner_global)
    return set_error(THEIA_HIP_ERR_UNSUPPORTED, "use_inner_iterations in a sharded solve needs theia_hip_ba_set_inner_global on every rank (or set it to 0 on every rank)");
  const bool inner = h->inner && O.use_inner_iterations != 0;
  st.inner_enabled = inner ? 1 : 0;
  LmState* dst = reinterpret_cast<LmState*>(h->lm_state.p);
  LmCtl ctl;
  ctl.max_iterations = O.max_num_iterations;
  ctl.trace_capacity = S->trace_cost ? S->trace_capacity : 0;
  ctl.function_tolerance = O.function_tolerance; ctl.gradient_tolerance = O.gradient_tolerance;
  ctl.parameter_tolerance = O.parameter_tolerance; ctl.max_radius = O.max_trust_region_radius; ctl.fixed_cost = h->fixed_cost;
  // the trace: its first kTraceHead entries behind the state, the rest (a longer trace only) in a block of its own
  const size_t tail = (size_t)std::max(0, ctl.trace_capacity - kTraceHead);
  if (tail > h->tr_tail_cap) {
    if ((rc = h->tr_tail.alloc(5 * tail))) return rc;
    h->tr_tail_cap = tail;
  }
  ctl.th = ctl.trace_capacity ? reinterpret_cast<double*>(h->lm_state.p + kLmStateBytes) : nullptr;
  ctl.tt = h->tr_tail.p; ctl.tt_cap = (int)h->tr_tail_cap;
  ctl.inner_scal = inner ? h->in_scal.p : nullptr;
  // the folded chain of glue launches: state and candidate buffers change roles on the device (LmState::cur), and the handle
  // puts its own pointers right again on EVERY way out of this function -- after the last read-back that succeeded
  const bool glue_run = lm_glue_run(h);
  struct Normalise {
    theia_ba_handle_s* h; LmState* st; bool on;
    void operator()() {
      if (!on || st->cur != 1) return;
      // the host's invariant "state = buffer 0" (download, snapshot, the queries, the next run): the buffers changed roles an
      // odd number of times; a replay graph captured on the old pointers is dropped with them
      h->cam[0].swap(h->cam[1]); h->pts[0].swap(h->pts[1]); h->camrot.swap(h->camrot_cand);
      h->P.camrot = h->camrot.p; h->P.camrot_cand = h->camrot_cand.p;
      h->drop_graph();
      st->cur = 0;
    }
    ~Normalise() { (*this)(); }
  } normalise{h, &st, glue_run};
  if (h->xnorm_part.n < 2 * (size_t)kXnormBlocks && (rc = h->xnorm_part.alloc(2 * kXnormBlocks))) return rc;
  // the initial state and the control block travel as kernel arguments: no host buffer whose lifetime would need a
  // synchronisation before the first iteration
  k_lm_init<<<1, 1, 0, h->stream>>>(dst, st, reinterpret_cast<LmCtl*>(h->lm_ctl.p), ctl, h->scalB.p);
  // |x| of the variable blocks at the start: summed on the device (points per shard, all-reduced)
  k_xnorm_partial<<<kXnormBlocks, 256, 0, h->stream>>>(h->P, h->cam[0].p, h->pts[0].p, h->intr[0].p, h->xnorm_part.p);
  if (h->allreduce) {
    k_xnorm_reduce<<<1, 1, 0, h->stream>>>(h->xnorm_part.p, kXnormBlocks, h->scalB.p);
    if ((rc = do_allreduce(h, h->scalB.p, 1, THEIA_REDUCE_SUM))) return rc;
    k_xnorm_set<<<1, 1, 0, h->stream>>>(dst, h->scalB.p);
  } else {
    k_xnorm_reduce_set<<<1, 1, 0, h->stream>>>(h->xnorm_part.p, kXnormBlocks, h->scalB.p, dst);
  }
  const LmCtl* dctl = reinterpret_cast<const LmCtl*>(h->lm_ctl.p);
  const int nxt = 1;
  // one LM iteration ("body"): linearise + Schur, solve, trial step, step control, accept
  auto enqueue_body = [&](int slot, bool first_fold = false, LmChain chain = LM_SEPARATE) -> int {
    const bool flip = chain != LM_SEPARATE;   // no k_lm_accept: an accepted step flips LmState::cur
    int r;
    if (slot >= 0) HIP_TRYR(hipEventRecord(h->ev[slot][0], h->stream));
    // (flip: the kernels pick state and candidate by LmState::cur; the first body runs at cur = 0, so its launches that do
    // not look -- the first-fold linearisation, k_cam_prep -- are right)
    struct CurScope { DevProblem& P; ~CurScope() { P.lm_cur = nullptr; P.pts_alt = nullptr; } } cur_scope{h->P};
    if (flip) { h->P.lm_cur = &dst->cur; h->P.pts_alt = h->pts[nxt].p; }
    if ((r = enqueue_linearize(h, slot, first_fold, chain))) return r;
    if (slot >= 0) HIP_TRYR(hipEventRecord(h->ev[slot][1], h->stream));
    const bool fuse = !h->allreduce && !inner && slot < 0 && h->ntiles_main > 0;   // tile reduction inside the control kernel
    if ((r = enqueue_solve_and_backsub(h, slot, fuse, chain))) return r;
    if (inner) {
      // DoInnerIterationsIfNeeded: one sweep of block coordinate descent on a copy of the candidate, its cost and its
      // distance from x; every kernel returns at once when the gate is closed (step invalid, inner iterations off, done)
      k_inner_gate<<<1, 1, 0, h->stream>>>(dst, h->rb.scal, h->scalB.p, h->in_gate.p);
      HIP_TRYR(hipMemcpyAsync(h->in_cam.p, h->cam[nxt].p, sizeof(double) * 6 * h->nc, hipMemcpyDeviceToDevice, h->stream));
      HIP_TRYR(hipMemcpyAsync(h->in_pts.p, h->pts[nxt].p, sizeof(double) * 4 * h->np, hipMemcpyDeviceToDevice, h->stream));
      HIP_TRYR(hipMemcpyAsync(h->in_intr.p, (h->ni ? h->intr[nxt].p : h->intr[0].p), sizeof(double) * THEIA_MAX_INTRINSICS * h->ng, hipMemcpyDeviceToDevice, h->stream));
      InnerArgs IA;
      IA.P = h->P;
      IA.cam_obs_off = h->in_cam_off.p; IA.cam_obs_idx = h->in_cam_idx.p; IA.grp_obs_off = h->in_grp_off.p; IA.grp_obs_idx = h->in_grp_idx.p;
      IA.trk_off = h->in_trk_off.p; IA.ntracks = h->in_ntracks; IA.nobs = h->nobs_main;
      IA.cam = h->in_cam.p; IA.pts = h->in_pts.p; IA.intr = h->in_intr.p; IA.gate = h->in_gate.p;
      IA.grp_part = h->in_grp_part.p; IA.grp_bar = h->in_grp_bar.p; IA.grp_wgs = h->in_grp_part.p ? inner_group_wgs(h->ng) : 1;
      if (h->allreduce && h->inner_global) {
        // the full candidate point set: every shard's points at their global indices, summed over the ranks
        HIP_TRYR(hipMemsetAsync(h->g_pts.p, 0, sizeof(double) * 4 * (size_t)h->g_np, h->stream));
        launch_inner_scatter_points(h->np, h->in_pts.p, h->g_pidx.p, h->g_pts.p, h->stream);
        if ((r = do_allreduce(h, h->g_pts.p, (size_t)4 * h->g_np, THEIA_REDUCE_SUM))) return r;
        InnerArgs IG = IA;      // cameras and groups over the full observation set, identically on every rank
        IG.P.obs_uv = h->g_uv.p; IG.P.obs_si = h->g_si.n ? h->g_si.p : nullptr; IG.P.obs_cam = h->g_cam.p; IG.P.obs_pt = h->g_pt.p;
        IG.P.obs_kind = h->g_kind.n ? h->g_kind.p : nullptr; IG.P.np = h->g_np; IG.P.nobs = h->g_nobs;
        IG.P.n_priors = h->g_npriors; IG.P.prior_cam = h->g_prior_cam.p; IG.P.prior_kind = h->g_prior_kind.p;
        IG.P.prior_vec = h->g_prior_vec.p; IG.P.prior_info = h->g_prior_info.p;
        IG.cam_obs_off = h->g_cam_off.p; IG.cam_obs_idx = h->g_cam_idx.p; IG.grp_obs_off = h->g_grp_off.p; IG.grp_obs_idx = h->g_grp_idx.p;
        IG.pts = h->g_pts.p; IG.ntracks = 0; IG.nobs = h->g_nobs;
        // with the shard geometry known the cameras (then the groups) are dealt to the ranks by index and the results summed
        // (the non-owned entries zeroed: x + 0 is exact, every rank ends with the same bits); otherwise every rank sweeps all
        const bool deal = h->shard_world > 1 && h->shard_rank >= 0 && h->shard_rank < h->shard_world;
        if (deal) { IG.own_rank = h->shard_rank; IG.own_world = h->shard_world; }
        launch_inner_sweep(IG, h->stream, 1);
        if (deal) {
          launch_inner_keep_owned(h->in_cam.p, h->nc, 6, h->shard_rank, h->shard_world, h->stream);
          if ((r = do_allreduce(h, h->in_cam.p, (size_t)6 * h->nc, THEIA_REDUCE_SUM))) return r;
        }
        if (h->ni > 0) {
          launch_inner_sweep(IG, h->stream, 2);
          if (deal) {
            launch_inner_keep_owned(h->in_intr.p, h->ng, THEIA_MAX_INTRINSICS, h->shard_rank, h->shard_world, h->stream);
            if ((r = do_allreduce(h, h->in_intr.p, (size_t)THEIA_MAX_INTRINSICS * h->ng, THEIA_REDUCE_SUM))) return r;
          }
        }
        launch_inner_sweep(IA, h->stream, 4);   // this shard's tracks against the swept cameras
        launch_inner_norms(IA, h->cam[0].p, h->pts[0].p, h->intr[0].p, h->g_stage.p, h->in_part.p, h->stream, 1);
        launch_inner_cost(IA, h->in_part.p, h->g_stage.p + 2, h->stream);
        if ((r = do_allreduce(h, h->g_stage.p, 4, THEIA_REDUCE_SUM))) return r;
        launch_inner_norms(IA, h->cam[0].p, h->pts[0].p, h->intr[0].p, h->g_stage.p + 4, h->in_part.p, h->stream, 2);
        launch_inner_combine(h->g_stage.p, h->g_stage.p + 4, h->in_scal.p, h->stream);
      } else {
      launch_inner_sweep(IA, h->stream);
      launch_inner_norms_cost(IA, h->cam[0].p, h->pts[0].p, h->intr[0].p, h->in_scal.p, h->in_part.p, h->stream);   // step norms + cost, two launches
      }
    }
    if (slot >= 0) HIP_TRYR(hipEventRecord(h->ev[slot][3], h->stream));
    const bool two_stage = h->ntiles_main > 4 * kReduceBlocks;
    double* clear16 = flip ? h->rb.scal : nullptr;
    if (fuse && two_stage) {
      launch_reduce_tiles_stage1(h->ntiles_main, h->tile_part.p, 5, h->fmaxflag.p + 8, h->red_part.p, h->stream);
      k_reduce_control<<<1, 1024, 0, h->stream>>>(kReduceBlocks, h->red_part.p, h->f2s.p + 8, h->fmaxflag.p + 8, dst, h->rb.scal, h->scalB.p, dctl, clear16, flip ? 1 : 0);
    } else if (fuse) k_reduce_control<<<1, 1024, 0, h->stream>>>(h->ntiles_main, h->tile_part.p, h->f2s.p + 8, h->fmaxflag.p + 8, dst, h->rb.scal, h->scalB.p, dctl, clear16, flip ? 1 : 0);
    else k_lm_control<<<1, 1, 0, h->stream>>>(dst, h->rb.scal, h->scalB.p, dctl);
    if (!flip)
    k_lm_accept<<<256, 256, 0, h->stream>>>(dst, h->cam[0].p, h->cam[nxt].p, (size_t)6 * h->nc, h->pts[0].p, h->pts[nxt].p,
                                            (size_t)4 * h->np, h->intr[0].p, h->intr[nxt].p, h->ni ? (size_t)THEIA_MAX_INTRINSICS * h->ng : 0,
                                            h->in_cam.p, h->in_pts.p, h->in_intr.p,
                                            (h->use_fused && h->ni == 0 && !h->inner) ? h->camrot.p : nullptr, h->camrot_cand.p, (size_t)40 * h->nc);
    return 0;
  };
  // Phase timing (HIP events around the kernel groups) is opt-in: THEIA_HIP_PHASE_TIMING=1.
  // Otherwise, and without an all-reduce callback, the body is captured ONCE into a hipGraph
  // and replayed: ~45 launches per iteration cost more host time than the GPU needs to run them.
  const bool timing = getenv("THEIA_HIP_PHASE_TIMING") != nullptr;
  const char* genv = getenv("THEIA_HIP_LM_GRAPH");
  // hipGraph replay is opt-in (THEIA_HIP_LM_GRAPH=1): it measured no faster than direct launches (the iteration
  // is bounded by the dependent kernels, not by host enqueue time), and a stream capture in one host thread makes
  // legacy-stream calls of other threads fail ("would make the legacy stream depend on a capturing blocking
  // stream") -- the entry points must stay callable concurrently from a thread pool.
  const bool want_graph = !timing && !h->allreduce && !inner && !h->graph_failed && (genv && genv[0] == '1');
  if (want_graph && !h->graph_exec) {
    bool ok = hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
    if (ok) {
      const int r = enqueue_body(-1);
      hipGraph_t g = nullptr;
      const hipError_t e = hipStreamEndCapture(h->stream, &g);
      ok = (r == 0) && e == hipSuccess && g != nullptr;
      if (ok) { h->graph = g; ok = hipGraphInstantiate(&h->graph_exec, g, nullptr, nullptr, 0) == hipSuccess; }
      else if (g) (void)hipGraphDestroy(g);
    }
    if (!ok) { h->drop_graph(); h->graph_failed = true; (void)hipGetLastError(); }
  }
  const bool use_graph = want_graph && h->graph_exec;
  // Several bodies are enqueued per synchronisation; bodies after termination are no-ops for
  // the state (k_lm_control returns at once) -- their kernels run on unchanged data.
  const char* chunk_env = getenv("THEIA_HIP_LM_CHUNK");
  int chunk = chunk_env ? atoi(chunk_env) : 4;
  chunk = std::max(1, std::min(chunk, (int)theia_ba_handle_s::kMaxChunk));
  const long long bodies_max = std::max(1, O.max_num_iterations);
  if (bodies_max <= theia_ba_handle_s::kMaxChunk && !chunk_env) chunk = (int)bodies_max;
  long long bodies_enqueued = 0;
  while (true) {
    {
      // max_solver_time_in_seconds: every other LM decision comes from all-reduced device state, so in a sharded solve
      // this one is made collective too (MAX over the ranks' own clocks) -- a rank that stopped alone would leave the
      // others waiting in their next all-reduce.
      double expired = (now_s() - t_start >= O.max_solver_time_in_seconds && bodies_enqueued > 0) ? 1.0 : 0.0;
      if (h->allreduce && bodies_enqueued > 0) {
        if (h->stop_flag.n < 8 && (rc = h->stop_flag.alloc(8))) return rc;
        h->h_scal[32] = expired;
        HIP_TRYR(hipMemcpyAsync(h->stop_flag.p, h->h_scal + 32, sizeof(double), hipMemcpyHostToDevice, h->stream));
        if ((rc = do_allreduce(h, h->stop_flag.p, 1, THEIA_REDUCE_MAX))) return rc;
        HIP_TRYR(hipMemcpyAsync(h->h_scal + 33, h->stop_flag.p, sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRYR(hipStreamSynchronize(h->stream));
        expired = h->h_scal[33];
      }
      if (expired != 0.0) { st.term = THEIA_TERM_NO_CONVERGENCE; break; }
    }
    const int nb = (int)std::min<long long>(chunk, bodies_max - bodies_enqueued);
    if (nb <= 0) break;
    for (int b = 0; b < nb; ++b) {
      if (use_graph) HIP_TRYR(hipGraphLaunch(h->graph_exec, h->stream));
      else {   // (first: a host-side fact -- bodies are enqueued ahead of the device)
        const bool first = bodies_enqueued == 0 && b == 0;
        if ((rc = enqueue_body(timing ? b : -1, fold && first, glue_run ? (first ? LM_FOLD_FIRST : LM_FOLDED) : LM_SEPARATE))) return rc;
      }
    }
    bodies_enqueued += nb;
    HIP_TRYR(hipGetLastError());   // a rejected launch configuration would otherwise go unnoticed
    // read-back through the handle's pinned block: an asynchronous copy needs a peer that outlives the call (HIP may
    // pin pageable pages and run the DMA later; stack temporaries were the round-1 corruption)
    // (with a trace: the state and the trace head behind it in the one copy)
    HIP_TRYR(hipMemcpyAsync(h->h_state, dst, ctl.trace_capacity ? kLmBlockBytes : sizeof(st), hipMemcpyDeviceToHost, h->stream));
    HIP_TRYR(hipStreamSynchronize(h->stream));
    std::memcpy(&st, h->h_state, sizeof(st));
    const int ran = (int)std::min<long long>(nb, std::max<long long>(0, (long long)st.bodies - (bodies_enqueued - nb)));
    for (int b = 0; timing && b < ran; ++b) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, h->ev[b][0], h->ev[b][1]) == hipSuccess) S->time_linearize += ms * 1e-3;
      if (hipEventElapsedTime(&ms, h->ev[b][1], h->ev[b][2]) == hipSuccess) S->time_solve_reduced += ms * 1e-3;
      if (hipEventElapsedTime(&ms, h->ev[b][2], h->ev[b][3]) == hipSuccess) S->time_backsub += ms * 1e-3;
      if (hipEventElapsedTime(&ms, h->ev[b][4], h->ev[b][5]) == hipSuccess) S->time_kernel_linearize += ms * 1e-3;
      S->num_linearize_launches++;
    }
    if (st.done) break;
  }
  normalise();   // before anything else looks at the handle's buffers: the extra linearisation below, download, the queries
  if (ctl.trace_capacity && st.pending_grad >= 0 && st.term != THEIA_TERM_FAILURE) {
    // the last step was accepted at the iteration cap (or the time ran out after it): the gradient its trace entry reports
    // is the one at the accepted point (ceres evaluates it as part of the successful step), so linearise there once more
    if ((rc = enqueue_linearize(h, -1, false))) return rc;
    k_lm_pending_gradient<<<1, 1, 0, h->stream>>>(dst, h->rb.scal, dctl);
    HIP_TRYR(hipMemcpyAsync(h->h_state, dst, kLmBlockBytes, hipMemcpyDeviceToHost, h->stream));   // the head again, with that entry
    HIP_TRYR(hipStreamSynchronize(h->stream));
  }
  if (ctl.trace_capacity) {
    // the stream has drained: the head is read from the handle's pinned block, only a longer trace copies its rest
    const int k = std::min(st.trace_size, S->trace_capacity);
    S->trace_size = k;
    const int kh = std::min(k, kTraceHead), kt = k - kh;
    void* out[5] = {S->trace_cost, S->trace_gradient_max_norm, S->trace_step_norm, S->trace_radius, S->trace_accepted};
    for (int a = 0; a < 5 && k; ++a) {
      if (!out[a]) continue;
      const size_t es = a == 4 ? sizeof(int) : sizeof(double);
      std::memcpy(out[a], h->h_state + kLmStateBytes + sizeof(double) * kTraceHead * a, es * kh);
      if (kt) HIP_TRYR(hipMemcpy(static_cast<char*>(out[a]) + es * kh, h->tr_tail.p + (size_t)a * h->tr_tail_cap, es * kt, hipMemcpyDeviceToHost));
    }
  }
  if (O.verbose)
    for (int k = 0; k < S->trace_size; ++k)
      std::fprintf(stderr, "[theia_hip] %3d cost %.6e |g| %.3e |step| %.3e radius %.3e %s\n", k, S->trace_cost[k],
                   S->trace_gradient_max_norm ? S->trace_gradient_max_norm[k] : 0.0, S->trace_step_norm ? S->trace_step_norm[k] : 0.0,
                   S->trace_radius ? S->trace_radius[k] : 0.0, (S->trace_accepted && S->trace_accepted[k]) ? "ok" : "rej");
  S->num_iterations = st.iter;
  S->num_successful_steps = st.num_successful;
  S->termination_type = st.term;
  S->success = st.term != THEIA_TERM_FAILURE;
  S->initial_cost = st.initial_cost;
  S->final_cost = st.fail_at_first ? st.initial_cost : st.minimum_cost + h->fixed_cost;
  h->stage.release();   // (the stream has been waited for: create()'s staged uploads are done)
  S->solve_time_in_seconds = now_s() - t_start;
  return 0;
}

int theia_hip_ba_solve(const theia_ba_problem* problem, const theia_ba_options* options, theia_ba_summary* summary) {
  if (!summary) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null summary");
  if (problem && options && (problem->flags & THEIA_BA_FLAG_INVERSE_DEPTH)) {
    const int vrc = validate(problem, options);
    return vrc ? vrc : ba_solve_inverse_depth(problem, options, summary);
  }
  const double t0 = now_s();
  theia_ba_handle h = nullptr;
  int rc = theia_hip_ba_create(problem, options, &h);
  if (rc) return rc;
  const double t1 = now_s();
  rc = theia_hip_ba_run(h, summary);
  const double t2 = now_s();
  if (!rc) rc = theia_hip_ba_download(h, const_cast<theia_ba_problem*>(problem));
  const double t3 = now_s();
  summary->setup_time_in_seconds = t1 - t0;
  theia_hip_ba_destroy(h);
  if (getenv("THEIA_HIP_CREATE_TIMING"))
    fprintf(stderr, "theia_hip ba_solve: create %.2f ms, run %.2f ms, download %.2f ms, destroy %.2f ms\n", 1e3 * (t1 - t0), 1e3 * (t2 - t1),
            1e3 * (t3 - t2), 1e3 * (now_s() - t3));
  return rc;
}

}  // extern "C"
