// nonlinear_positions.hip -- NonlinearPositionEstimator (global_pose_estimation/nonlinear_position_estimator.{h,cc},
// pairwise_translation_error.{h,cc}): the Ceres Levenberg-Marquardt solve over PairwiseTranslationError with a Huber
// loss, on the device in FP64.  DESIGN.md 3.6l has the derivation.
//
// The graph has one node per view and one per track point, every node a 3-vector; node num_views + t is point t.  The
// edges are the camera-to-camera pairs in input order, then one point-to-camera edge per observation, from the
// observing view to the point.  Per edge (a, b) with d = x_b - x_a, direction t, weight w and scale s
// (pairwise_translation_error.h:65-100):
//   s > 0      r = w (d - s t),        dr/dx_b = w I
//   otherwise  r = w (d / nrm - t),    dr/dx_b = w (I - u u') / nrm, u = d / nrm, nrm = |d|;
//              nrm < 1e-12: nrm = 1, a constant (the Jet comparison replaces value and derivative), dr/dx_b = w I
// and dr/dx_a = -dr/dx_b throughout.  HuberLoss(a) on q = |r|^2 with b = a^2: rho = q, rho' = 1 while q <= b, else
// rho = 2 a sqrt(q) - b, rho' = max(DBL_MIN, a / sqrt(q)); rho'' <= 0 in both, so Ceres' corrector scales the residual
// and both blocks by sqrt(rho').
//
// k_directions (set-up, once) writes t, w, s per edge: t = R(w_i)' position_2, w = 1, s = scale_estimate for a pair;
// t = normalize(R(w_ray)' [x, y, 1]), w = point_to_camera_weight, s = -1 for an observation.  k_linearise and
// k_candidate are this file's; everything downstream of the 24-double edge record -- k_column_norms, k_gradient, k_post,
// k_assemble, the dense factorisation, k_step, k_decide -- is graph_lm.h's, shared with nonlinear_rotations.hip, whose
// header comment describes the loop.  Points are nodes of the dense system, not Schur-eliminated.
//
// Determinism: no atomics of this file's own.  Every sum has one owner and a fixed order.  Two runs on one input are
// bit-identical.
#include "rotation_maps.h"
#include "graph_lm.h"

#include <chrono>
#include <vector>

namespace thip {
namespace {

// One lane per edge: the direction, weight and scale of the edge.  E_cam pairs, then the observations.
__global__ __launch_bounds__(kThreads) void k_directions(int E, int E_cam, const int2* __restrict__ edges,
                                                         const double* __restrict__ orientations,
                                                         const double* __restrict__ ray_orientations,
                                                         const double* __restrict__ rel, const double* __restrict__ scale_est,
                                                         const double* __restrict__ feature, double point_weight,
                                                         double* __restrict__ dir, double* __restrict__ ws) {
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= E) return;
  const bool pair = e < E_cam;
  const int view = edges[e].x;
  double R[9], v[3], w, s;
  if (pair) {
    rsc::angle_axis_to_rot(orientations + 3 * (size_t)view, R);
    v[0] = rel[3 * (size_t)e]; v[1] = rel[3 * (size_t)e + 1]; v[2] = rel[3 * (size_t)e + 2];
    w = 1.0;
    s = scale_est ? scale_est[e] : -1.0;
  } else {
    const size_t o = (size_t)(e - E_cam);
    rsc::angle_axis_to_rot(ray_orientations + 3 * (size_t)view, R);
    v[0] = feature[2 * o]; v[1] = feature[2 * o + 1]; v[2] = 1.0;
    w = point_weight;
    s = -1.0;
  }
  double t[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) t[c] = (R[c] * v[0] + R[3 + c] * v[1]) + R[6 + c] * v[2];
  if (!pair) {
    const double nrm = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
    t[0] /= nrm; t[1] /= nrm; t[2] /= nrm;
  }
  dir[3 * (size_t)e] = t[0]; dir[3 * (size_t)e + 1] = t[1]; dir[3 * (size_t)e + 2] = t[2];
  ws[2 * (size_t)e] = w; ws[2 * (size_t)e + 1] = s;
}

// What k_linearise and k_candidate share: the residual, the branch it took, and HuberLoss at |r|^2 (rho and
// sqrt(rho')).  One code path, so that an accepted candidate's cost is the cost of its linearisation.
enum { kBranchScaled = 0, kBranchNormalised = 1, kBranchTiny = 2 };
struct EdgeEval {
  double r[3], u[3], nrm, rho, sr;
  int branch;
};
__device__ __forceinline__ void edge_eval(const double* xa, const double* xb, const double* t, double w, double s,
                                          double a, double b, EdgeEval& v) {
  const double d0 = xb[0] - xa[0], d1 = xb[1] - xa[1], d2 = xb[2] - xa[2];
  if (s > 0.0) {
    v.branch = kBranchScaled;
    v.nrm = 1.0;
    v.u[0] = v.u[1] = v.u[2] = 0.0;
    v.r[0] = w * (d0 - s * t[0]); v.r[1] = w * (d1 - s * t[1]); v.r[2] = w * (d2 - s * t[2]);
  } else {
    double nrm = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
    v.branch = kBranchNormalised;
    if (nrm < 1e-12) { nrm = 1.0; v.branch = kBranchTiny; }
    v.nrm = nrm;
    v.u[0] = d0 / nrm; v.u[1] = d1 / nrm; v.u[2] = d2 / nrm;
    v.r[0] = w * (v.u[0] - t[0]); v.r[1] = w * (v.u[1] - t[1]); v.r[2] = w * (v.u[2] - t[2]);
  }
  const double q = (v.r[0] * v.r[0] + v.r[1] * v.r[1]) + v.r[2] * v.r[2];
  if (q <= b) {
    v.rho = q;
    v.sr = 1.0;
  } else {
    const double sq = sqrt(q);
    v.rho = 2.0 * a * sq - b;
    v.sr = sqrt(fmax(DBL_MIN, a / sq));
  }
}

// One lane per edge: the record rec[e] = (Js_a, Js_b, corrected residual) at x, and the blocks' sums of rho.  An edge
// between two held views is not in the problem (Ceres drops a residual block whose parameter blocks are all constant).
__global__ __launch_bounds__(kThreads) void k_linearise(int E, const int2* __restrict__ edges, const int* __restrict__ idx,
                                                        const double* __restrict__ x, const double* __restrict__ dir,
                                                        const double* __restrict__ ws, const double* __restrict__ scale,
                                                        double a, double b, double* __restrict__ rec,
                                                        double* __restrict__ part_cost, const NlState* __restrict__ st) {
  __shared__ double red[kThreads];
  if (st->done || !st->fresh) return;
  const int e = blockIdx.x * kThreads + threadIdx.x;
  double rho = 0.0;
  if (e < E) {
    const int2 ij = edges[e];
    const int fa = idx[ij.x], fb = idx[ij.y];
    if (fa >= 0 || fb >= 0) {
      double xa[3], xb[3], t[3], sa[3] = {0.0, 0.0, 0.0}, sb[3] = {0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        xa[k] = x[3 * (size_t)ij.x + k]; xb[k] = x[3 * (size_t)ij.y + k]; t[k] = dir[3 * (size_t)e + k];
        if (fa >= 0) sa[k] = scale[3 * (size_t)fa + k];
        if (fb >= 0) sb[k] = scale[3 * (size_t)fb + k];
      }
      const double w = ws[2 * (size_t)e];
      EdgeEval v;
      edge_eval(xa, xb, t, w, ws[2 * (size_t)e + 1], a, b, v);
      rho = v.rho;
      // dr/dx_b = w (I - u u') / nrm: u = 0 and nrm = 1 in the scaled branch; the tiny-norm branch is w I as well
      const bool project = v.branch == kBranchNormalised;
      double* o = rec + kRec * (size_t)e;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double eye = r == c ? 1.0 : 0.0;
          const double m = (project ? w * (eye - v.u[r] * v.u[c]) / v.nrm : w * eye) * v.sr;
          o[3 * r + c] = -m * sa[c];
          o[9 + 3 * r + c] = m * sb[c];
        }
        o[18 + r] = v.r[r] * v.sr;
      }
    }
  }
  const double s = block_sum<kThreads>(rho, red);
  if (threadIdx.x == 0) part_cost[blockIdx.x] = s;
}

// One lane per edge: rho at the candidate, and the model cost change -m . (r + m / 2) with m = -Js y from the record.
__global__ __launch_bounds__(kThreads) void k_candidate(int E, const int2* __restrict__ edges, const int* __restrict__ idx,
                                                        const double* __restrict__ xc, const double* __restrict__ dir,
                                                        const double* __restrict__ ws, const double* __restrict__ rec,
                                                        const double* __restrict__ y, double a, double b,
                                                        double* __restrict__ part, const NlState* __restrict__ st) {
  __shared__ double red[kThreads];
  if (st->done) return;
  const int e = blockIdx.x * kThreads + threadIdx.x;
  double rho = 0.0, model = 0.0;
  if (e < E) {
    const int2 ij = edges[e];
    const int fa = idx[ij.x], fb = idx[ij.y];
    if (fa >= 0 || fb >= 0) {
      double xa[3], xb[3], t[3], ya[3], yb[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        xa[k] = xc[3 * (size_t)ij.x + k]; xb[k] = xc[3 * (size_t)ij.y + k]; t[k] = dir[3 * (size_t)e + k];
        ya[k] = fa >= 0 ? -y[3 * (size_t)fa + k] : 0.0;
        yb[k] = fb >= 0 ? -y[3 * (size_t)fb + k] : 0.0;
      }
      EdgeEval v;
      edge_eval(xa, xb, t, ws[2 * (size_t)e], ws[2 * (size_t)e + 1], a, b, v);
      rho = v.rho;
      const double* R = rec + kRec * (size_t)e;
      double s = 0.0;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double mi = (R[3 * r] * ya[0] + R[3 * r + 1] * ya[1]) + R[3 * r + 2] * ya[2];
        const double mj = (R[9 + 3 * r] * yb[0] + R[9 + 3 * r + 1] * yb[1]) + R[9 + 3 * r + 2] * yb[2];
        const double mr = mi + mj;
        s += mr * (R[18 + r] + mr / 2.0);
      }
      model = -s;
    }
  }
  const double s0 = block_sum<kThreads>(rho, red), s1 = block_sum<kThreads>(model, red);
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = s0; part[2 * blockIdx.x + 1] = s1; }
}

bool all_finite(const double* p, size_t n) {
  for (size_t k = 0; k < n; ++k)
    if (!std::isfinite(p[k])) return false;
  return true;
}

}  // namespace
}  // namespace thip

using namespace thip;

extern "C" int theia_hip_nonlinear_positions(int32_t num_views, const double* orientations, double* positions,
                                             const uint8_t* fixed, int32_t num_edges, const int32_t* edges,
                                             const double* relative_translations, const double* scale_estimates,
                                             int32_t num_points, double* points, const int32_t* track_offsets,
                                             const int32_t* obs_view, const double* obs_feature,
                                             const double* ray_orientations, double point_to_camera_weight,
                                             const theia_nonlinear_position_options* options,
                                             theia_nonlinear_position_summary* summary, double* trace_out,
                                             int32_t trace_capacity) {
  const auto t_start = std::chrono::steady_clock::now();
  const int n = num_views, Ec = num_edges, T = num_points;
  if (!summary) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null summary");
  *summary = theia_nonlinear_position_summary{};
  theia_nonlinear_position_options o{400, 0, 0.1, 1e-6, 1e-10, 1e-8, 1e16};
  if (options) o = *options;
  // ---- refusals, before the device is touched
  if (n < 1 || !orientations || !positions) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "no views, or null orientations / positions");
  if (Ec < 0 || (Ec > 0 && (!edges || !relative_translations))) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "bad camera-to-camera edges");
  if (T < 0 || (T > 0 && (!points || !track_offsets))) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "num_points > 0 with a null array");
  if (T > 0 && track_offsets[0] != 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "track_offsets[0] must be 0");
  for (int t = 0; t < T; ++t)
    if (track_offsets[t + 1] <= track_offsets[t])
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "track_offsets do not increase at track %d", t);
  const int Eo = T > 0 ? track_offsets[T] : 0;
  if (Eo > 0 && (!obs_view || !obs_feature)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "observations with a null array");
  if ((long long)Ec + Eo < 1) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "no edges of either kind");
  if ((long long)Ec + Eo > INT32_MAX / 2 || (long long)n + T > INT32_MAX / 4) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "too many edges or nodes");
  if (trace_capacity < 0 || (trace_capacity > 0 && !trace_out)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "bad trace buffer");
  if (o.max_num_iterations < 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "max_num_iterations must be >= 0");
  if (!positive_finite(o.robust_loss_width)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "robust_loss_width must be positive and finite");
  if (!positive_finite(point_to_camera_weight)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "point_to_camera_weight must be positive and finite");
  if (!nonnegative_finite(o.function_tolerance) || !nonnegative_finite(o.gradient_tolerance) ||
      !nonnegative_finite(o.parameter_tolerance))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "the tolerances must be finite and not negative");
  if (!positive_finite(o.max_trust_region_radius))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "max_trust_region_radius must be positive and finite");
  const int N = n + T, E = Ec + Eo;
  std::vector<int32_t> all_edges(2 * (size_t)E);
  for (int e = 0; e < Ec; ++e) {
    const int i = edges[2 * e], j = edges[2 * e + 1];
    if (i < 0 || i >= n || j < 0 || j >= n) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "edge %d names a view out of range", e);
    if (i == j)   // Ceres refuses a residual block that names one parameter block twice
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "edge %d joins view %d to itself", e, i);
    all_edges[2 * (size_t)e] = i; all_edges[2 * (size_t)e + 1] = j;
  }
  {
    std::vector<int> seen(n, -1);   // the last track that named the view
    for (int t = 0; t < T; ++t)
      for (int k = track_offsets[t]; k < track_offsets[t + 1]; ++k) {
        const int v = obs_view[k];
        if (v < 0 || v >= n) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "observation %d names a view out of range", k);
        if (seen[v] == t) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "track %d names view %d twice", t, v);
        seen[v] = t;
        all_edges[2 * ((size_t)Ec + k)] = v; all_edges[2 * ((size_t)Ec + k) + 1] = n + t;
      }
  }
  if (!all_finite(orientations, 3 * (size_t)n) || !all_finite(positions, 3 * (size_t)n) ||
      !all_finite(relative_translations, 3 * (size_t)Ec) || (scale_estimates && !all_finite(scale_estimates, Ec)) ||
      (T > 0 && !all_finite(points, 3 * (size_t)T)) || !all_finite(obs_feature, 2 * (size_t)Eo) ||
      (ray_orientations && !all_finite(ray_orientations, 3 * (size_t)n)))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "a non-finite input");

  std::vector<uint8_t> out(N, 1);   // the nodes that take no columns: held views, views without an edge
  for (int e = 0; e < E; ++e) out[all_edges[2 * (size_t)e]] = out[all_edges[2 * (size_t)e + 1]] = 0;
  for (int v = 0; v < n && fixed; ++v) if (fixed[v]) out[v] = 1;
  ViewGraphPlan g;
  fill_view_graph_lists(N, out, E, all_edges.data(), &g);
  const int m = g.m;
  theia_nonlinear_position_summary sm{};
  for (int v = 0; v < n; ++v) sm.num_views_in_problem += g.idx[v] >= 0;
  sm.num_points_in_problem = T;
  for (int e = 0; e < Ec; ++e) sm.num_camera_edges_in_problem += g.idx[edges[2 * e]] >= 0 || g.idx[edges[2 * e + 1]] >= 0;
  sm.num_point_edges_in_problem = Eo;
  if (m == 0) {   // every view of every edge is held and there is no point: nothing to solve
    sm.seconds = ms_since(t_start) * 1e-3;
    *summary = sm;
    return 0;
  }
  if ((long long)m * 3 + 1 > INT32_MAX / 2) return set_error(THEIA_HIP_ERR_OUT_OF_MEMORY, "%d nodes: the dense system does not fit", m);
  const int n3 = 3 * m;

  int rc;
  if ((rc = thip::ensure_device())) return rc;
  hipStream_t st = nullptr;
  const int nbE = grid_of(E, kThreads), nbM = grid_of(m, kThreads), nbV = grid_of(m, kViewsPerBlock);
  const int rows = o.max_num_iterations + 1;
  DenseSpd A;   // row n3: the right-hand side
  DeviceViewGraph dg;
  DevBuf<double> d_x, d_xc, d_or, d_ray, d_rel, d_se, d_feat, d_dir, d_ws, d_rec, d_scale, d_g, d_y, d_pc, d_pg, d_pcand,
      d_pstep, d_trace;
  DevBuf<NlState> d_st;
  const std::vector<double> ones(n3, 1.0);
  std::vector<double> x0(3 * (size_t)N);
  std::copy(positions, positions + 3 * (size_t)n, x0.begin());
  if (T > 0) std::copy(points, points + 3 * (size_t)T, x0.begin() + 3 * (size_t)n);
  // the dense system first: when it does not fit, that is the answer
  if ((rc = A.alloc(n3, 1)) || (rc = d_x.up(x0.data(), x0.size())) || (rc = d_xc.up(x0.data(), x0.size())) ||
      (rc = d_or.up(orientations, 3 * (size_t)n)) || (rc = d_ray.up(ray_orientations, ray_orientations ? 3 * (size_t)n : 0)) ||
      (rc = d_rel.up(relative_translations, 3 * (size_t)Ec)) || (rc = d_se.up(scale_estimates, scale_estimates ? Ec : 0)) ||
      (rc = d_feat.up(obs_feature, 2 * (size_t)Eo)) || (rc = dg.up(g, all_edges.data(), E, N)) ||
      (rc = d_dir.alloc(3 * (size_t)E)) || (rc = d_ws.alloc(2 * (size_t)E)) || (rc = d_rec.alloc(kRec * (size_t)E)) ||
      (rc = d_scale.up(ones.data(), n3)) || (rc = d_g.alloc(n3)) || (rc = d_y.alloc(n3)) || (rc = d_pc.alloc(nbE)) ||
      (rc = d_pg.alloc(nbV)) || (rc = d_pcand.alloc(2 * (size_t)nbE)) || (rc = d_pstep.alloc(2 * (size_t)nbM)) ||
      (rc = d_trace.alloc(5 * (size_t)rows)) || (rc = d_st.alloc(1)))
    return rc;
  const ViewGraphLists& vg = dg.lists;

  NlState hs{};
  lm::start(hs); hs.fresh = 1;
  HIP_TRY(hipMemcpy(d_st.p, &hs, sizeof(NlState), hipMemcpyHostToDevice));
  HIP_TRY(hipMemsetAsync(A.flag(), 0, sizeof(double), st));
  HIP_TRY(hipMemsetAsync(d_rec.p, 0, sizeof(double) * kRec * (size_t)E, st));
  const double a = o.robust_loss_width, b = a * a;
  const int* done = &d_st.p->done;
  k_directions<<<nbE, kThreads, 0, st>>>(E, Ec, vg.edges, d_or.p, ray_orientations ? d_ray.p : d_or.p, d_rel.p,
                                         scale_estimates ? d_se.p : nullptr, d_feat.p, point_to_camera_weight, d_dir.p,
                                         d_ws.p);

  auto linearise = [&]() {
    k_linearise<<<nbE, kThreads, 0, st>>>(E, vg.edges, vg.idx, d_x.p, d_dir.p, d_ws.p, d_scale.p, a, b, d_rec.p, d_pc.p, d_st.p);
  };
  auto gradient_and_post = [&](int init) {
    k_gradient<<<nbV, kThreads, 0, st>>>(vg, d_rec.p, d_scale.p, d_g.p, d_pg.p, d_st.p);
    k_post<<<1, kThreads, 0, st>>>(init, m, vg.free_view, d_x.p, d_pc.p, nbE, d_pg.p, nbV, o.max_num_iterations,
                                   o.gradient_tolerance, d_trace.p, rows, THEIA_ROTATION_TERM_GRADIENT_TOLERANCE,
                                   THEIA_ROTATION_TERM_MAX_ITERATIONS, THEIA_ROTATION_TERM_MIN_RADIUS, d_st.p);
  };
  // ---- the first linearisation: unscaled, the Jacobi scaling from its columns, then scaled
  linearise();
  k_column_norms<<<nbV, kThreads, 0, st>>>(vg, d_rec.p, d_scale.p);
  linearise();
  gradient_and_post(1);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(&hs, d_st.p, sizeof(NlState), hipMemcpyDeviceToHost));

  // ---- the LM loop
  DecideArgs da{nbE, nbM, 3 * N, rows, THEIA_ROTATION_TERM_PARAMETER_TOLERANCE, THEIA_ROTATION_TERM_FUNCTION_TOLERANCE,
                THEIA_ROTATION_TERM_FAILURE, o.function_tolerance, o.parameter_tolerance, o.max_trust_region_radius};
  rc = run_until_done(o.max_num_iterations, lm_chunk_size(), d_st.p, &hs, [&]() {
    if (int bad = A.clear(st)) return bad;
    k_assemble<<<grid_of((size_t)m + g.P, kThreads), kThreads, 0, st>>>(vg, A.lda, d_rec.p, d_g.p, A.A(), d_st.p);
    A.factor(1, st, done);
    A.back_substitute(1, A.rhs_row(0), A.lda, d_y.p, st, done);
    k_step<<<nbM, kThreads, 0, st>>>(m, vg.free_view, d_x.p, d_scale.p, d_y.p, d_xc.p, d_pstep.p, d_st.p);
    k_candidate<<<nbE, kThreads, 0, st>>>(E, vg.edges, vg.idx, d_xc.p, d_dir.p, d_ws.p, d_rec.p, d_y.p, a, b, d_pcand.p, d_st.p);
    k_decide<<<1, kThreads, 0, st>>>(da, d_pcand.p, d_pstep.p, A.flag(), d_x.p, d_xc.p, d_trace.p, d_st.p);
    linearise();
    gradient_and_post(0);
    return 0;
  });
  if (rc) return rc;
  if (!hs.done) return set_error(THEIA_HIP_ERR_INTERNAL, "the loop ended without a termination");

  // ---- Ceres copies its state back unless the solve failed
  if (hs.term != THEIA_ROTATION_TERM_FAILURE) {
    std::vector<double> x(3 * (size_t)N);
    HIP_TRY(hipMemcpy(x.data(), d_x.p, sizeof(double) * x.size(), hipMemcpyDeviceToHost));
    for (int v = 0; v < N; ++v)
      if (g.idx[v] >= 0) {
        double* dst = v < n ? positions + 3 * (size_t)v : points + 3 * (size_t)(v - n);
        for (int c = 0; c < 3; ++c) dst[c] = x[3 * (size_t)v + c];
      }
  }
  const int have = std::min(hs.trace_rows, rows);
  sm.trace_size = std::min(have, (int)trace_capacity);
  if (sm.trace_size > 0)
    HIP_TRY(hipMemcpy(trace_out, d_trace.p, sizeof(double) * 5 * (size_t)sm.trace_size, hipMemcpyDeviceToHost));
  sm.iterations = hs.iterations;
  sm.num_successful_steps = hs.successful;
  sm.num_unsuccessful_steps = hs.unsuccessful;
  sm.num_invalid_steps = hs.invalid;
  sm.termination = hs.term;
  sm.initial_cost = hs.initial_cost;
  sm.final_cost = hs.cost;
  sm.final_radius = hs.radius;
  sm.final_gradient_max_norm = hs.gmax;
  sm.seconds = ms_since(t_start) * 1e-3;
  *summary = sm;
  return 0;
}
