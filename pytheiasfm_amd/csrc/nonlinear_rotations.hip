// nonlinear_rotations.hip -- NonlinearRotationEstimator (global_pose_estimation/nonlinear_rotation_estimator.{h,cc},
// pairwise_rotation_error.{h,cc}; pybind sfm.cc:1782-1787): the Ceres Levenberg-Marquardt solve over PairwiseRotationError
// with a SoftL1 loss, on the device in FP64.  DESIGN.md 3.6i has the derivation.
//
// Per pair e = (i, j) the residual is r_e = log(R(w_j) R(w_i)' R(rel_e)') as an angle-axis vector: three
// ceres::AngleAxisToRotationMatrix and one ceres::RotationMatrixToAngleAxis (through the quaternion), with the small-angle
// branches of both.  Its two 3 x 3 Jacobians are the chain rule through the branch actually taken -- what Ceres' Jets give
// (the maps and their derivatives: rotation_derivatives.h, shared with alignment.hip):
//   dR/dw_k      Rodrigues, R = c I + (1 - c) u u' + s [u]x, u = w / theta (theta^2 > eps), else I + [w]x
//   dE           dR_j,k (R_i' R_rel')  and  R_j (dR_i,k' R_rel')
//   dq           the quaternion of E by the trace branch (trace >= 0) or the largest-diagonal branch
//   dr           2 atan2(|v|, q0) v / |v| (|v|^2 > 0, with Ceres' sign handling for q0 < 0), else 2 v
// SoftLOneLoss(a) on s = |r|^2: rho'' < 0 everywhere, so Ceres' corrector scales residual and Jacobian by sqrt(rho').
//
// The LM loop is Ceres 2.2's TrustRegionMinimizer + LevenbergMarquardtStrategy on the dense normal
// equations of order 3m (m = the free views that have an edge).  k_linearise and k_candidate are this file's; the
// kernels downstream of the edge record are graph_lm.h's, shared with nonlinear_positions.hip:
//   k_linearise   one lane per edge: residual, Jacobians, corrector, Jacobi scaling -> the edge's record; cost per block
//   k_column_norms  first linearisation only, one wavefront per free view: scale = 1 / (1 + |column|)
//   k_gradient    one wavefront per free view: Js' r over its incident edges; max |g| per block
//   k_post        one workgroup: gradient max norm, the trace row, then cap / gradient tolerance / radius floor
//   k_assemble    lower triangle of Js'Js + D and the right-hand-side row, owner sums in edge order (view_graph_plan.h)
//   dense_cholesky_factor + dense_cholesky_back_substitute (the BA's K3 kernels), device fail flag
//   k_step        one lane per free view: candidate x - scale * y, |step|^2 and |candidate|^2 per block
//   k_candidate   one lane per edge: the candidate's cost term and the model cost change -m . (r + m / 2), m = -Js y
//   k_decide      one workgroup: Ceres' rules in Ceres' order; swaps the iterate on acceptance; raises `done`
// Every kernel returns at once while `done` is set; the host enqueues iterations in chunks and reads the state once per
// chunk (lud_positions.hip's pattern).  The factorisation is in place and fills the lower triangle, so the array is cleared
// before every assembly.
//
// theia_hip_selftest_pairwise_rotation_error at the bottom is test-only: k_selftest_edge runs linearise_edge, the per-edge
// body of k_linearise, on caller-supplied vectors, for tests/test_wide_rotations_gpu.py to compare with 50-digit values.
//
// Determinism: no atomics of this file's own (the factorisation's fail flag is the only one, and it is only compared with
// zero).  Every sum has one owner and a fixed order.  Two runs on one input are bit-identical.
#include "graph_lm.h"
#include "rotation_derivatives.h"   // aa_rot, log_rot and their derivatives
#include "small_linalg.h"

#include <chrono>
#include <vector>

namespace thip {
namespace {

// C = A' B', all row-major 3 x 3 (C = A B: rsc::matmul3)
__device__ __forceinline__ void mul33_tt(const double* A, const double* B, double* C) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) C[3 * r + c] = (A[r] * B[3 * c] + A[3 + r] * B[3 * c + 1]) + A[6 + r] * B[3 * c + 2];
}

// What k_linearise and k_candidate share: the rotations, E = R_j R_i' R_rel', r = log E, and SoftLOneLoss at |r|^2
// (rho and sqrt(rho')).  One code path, so that an accepted candidate's cost is the cost of its linearisation.
struct EdgeEval {
  AaCtx ci, cj, cr;
  double Rj[9], Rrel[9], M[9], Em[9], r[3], rho, sr;
  LogCtx L;
};
__device__ __forceinline__ void edge_eval(const double* wi, const double* wj, const double* wr, double b, EdgeEval& v) {
  double Ri[9];
  aa_rot(wi, v.ci, Ri);
  aa_rot(wj, v.cj, v.Rj);
  aa_rot(wr, v.cr, v.Rrel);
  mul33_tt(Ri, v.Rrel, v.M);
  rsc::matmul3(v.Rj, v.M, v.Em);
  log_rot(v.Em, v.L, v.r);
  const double s = (v.r[0] * v.r[0] + v.r[1] * v.r[1]) + v.r[2] * v.r[2];
  const double sq = sqrt(1.0 + s / b);
  v.rho = 2.0 * b * (sq - 1.0);
  v.sr = sqrt(1.0 / sq);
}

template <int K>
__device__ __forceinline__ void jacobian_columns(const EdgeEval& v, bool free_i, bool free_j, const double* si,
                                                 const double* sj, double* Ji, double* Jj) {
  double D[9], N[9], dE[9], dr[3];
  if (free_j) {
    aa_rot_d<K>(v.cj, D);
    rsc::matmul3(D, v.M, dE);
    log_rot_d(v.Em, dE, v.L, dr);
#pragma unroll
    for (int r = 0; r < 3; ++r) Jj[3 * r + K] = (dr[r] * v.sr) * sj[K];
  }
  if (free_i) {
    aa_rot_d<K>(v.ci, D);
    mul33_tt(D, v.Rrel, N);
    rsc::matmul3(v.Rj, N, dE);
    log_rot_d(v.Em, dE, v.L, dr);
#pragma unroll
    for (int r = 0; r < 3; ++r) Ji[3 * r + K] = (dr[r] * v.sr) * si[K];
  }
}

// The record of one edge at (wi, wj): o = (Js_i, Js_j, corrected residual), a held view's block left as it is.  Returns
// rho; `branch` is the branch the logarithm took (LogCtx).  k_linearise and the self-check entry at the bottom share it.
__device__ __forceinline__ double linearise_edge(const double* wi, const double* wj, const double* wr, bool free_i,
                                                 bool free_j, const double* si, const double* sj, double b,
                                                 double* __restrict__ o, int& branch) {
  EdgeEval v;
  edge_eval(wi, wj, wr, b, v);
  double Ji[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, Jj[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  jacobian_columns<0>(v, free_i, free_j, si, sj, Ji, Jj);
  jacobian_columns<1>(v, free_i, free_j, si, sj, Ji, Jj);
  jacobian_columns<2>(v, free_i, free_j, si, sj, Ji, Jj);
#pragma unroll
  for (int q = 0; q < 9; ++q) { o[q] = Ji[q]; o[9 + q] = Jj[q]; }
  o[18] = v.r[0] * v.sr; o[19] = v.r[1] * v.sr; o[20] = v.r[2] * v.sr;
  branch = v.L.branch;
  return v.rho;
}

// One lane per edge: the record rec[e] = (Js_i, Js_j, corrected residual) at x, and the blocks' sums of rho.  An edge
// between two held views is not in the problem (Ceres drops a residual block whose parameter blocks are all constant).
__global__ __launch_bounds__(kThreads) void k_linearise(int E, const int2* __restrict__ edges, const int* __restrict__ idx,
                                                        const double* __restrict__ x, const double* __restrict__ rel,
                                                        const double* __restrict__ scale, double b,
                                                        double* __restrict__ rec, double* __restrict__ part_cost,
                                                        const NlState* __restrict__ st) {
  __shared__ double red[kThreads];
  if (st->done || !st->fresh) return;
  const int e = blockIdx.x * kThreads + threadIdx.x;
  double rho = 0.0;
  if (e < E) {
    const int2 ij = edges[e];
    const int a = idx[ij.x], c = idx[ij.y];
    if (a >= 0 || c >= 0) {
      double wi[3], wj[3], wr[3], si[3] = {0.0, 0.0, 0.0}, sj[3] = {0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        wi[k] = x[3 * (size_t)ij.x + k]; wj[k] = x[3 * (size_t)ij.y + k]; wr[k] = rel[3 * (size_t)e + k];
        if (a >= 0) si[k] = scale[3 * (size_t)a + k];
        if (c >= 0) sj[k] = scale[3 * (size_t)c + k];
      }
      int branch;
      rho = linearise_edge(wi, wj, wr, a >= 0, c >= 0, si, sj, b, rec + kRec * (size_t)e, branch);
    }
  }
  const double s = block_sum<kThreads>(rho, red);
  if (threadIdx.x == 0) part_cost[blockIdx.x] = s;
}

// One lane per edge: rho at the candidate, and the model cost change -m . (r + m / 2) with m = -Js y from the record.
__global__ __launch_bounds__(kThreads) void k_candidate(int E, const int2* __restrict__ edges, const int* __restrict__ idx,
                                                        const double* __restrict__ xc, const double* __restrict__ rel,
                                                        const double* __restrict__ rec, const double* __restrict__ y,
                                                        double b, double* __restrict__ part, const NlState* __restrict__ st) {
  __shared__ double red[kThreads];
  if (st->done) return;
  const int e = blockIdx.x * kThreads + threadIdx.x;
  double rho = 0.0, model = 0.0;
  if (e < E) {
    const int2 ij = edges[e];
    const int a = idx[ij.x], c = idx[ij.y];
    if (a >= 0 || c >= 0) {
      double wi[3], wj[3], wr[3], yi[3], yj[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        wi[k] = xc[3 * (size_t)ij.x + k]; wj[k] = xc[3 * (size_t)ij.y + k]; wr[k] = rel[3 * (size_t)e + k];
        yi[k] = a >= 0 ? -y[3 * (size_t)a + k] : 0.0;
        yj[k] = c >= 0 ? -y[3 * (size_t)c + k] : 0.0;
      }
      EdgeEval v;
      edge_eval(wi, wj, wr, b, v);
      rho = v.rho;
      const double* R = rec + kRec * (size_t)e;
      double s = 0.0;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double mi = (R[3 * r] * yi[0] + R[3 * r + 1] * yi[1]) + R[3 * r + 2] * yi[2];
        const double mj = (R[9 + 3 * r] * yj[0] + R[9 + 3 * r + 1] * yj[1]) + R[9 + 3 * r + 2] * yj[2];
        const double mr = mi + mj;
        s += mr * (R[18 + r] + mr / 2.0);
      }
      model = -s;
    }
  }
  const double s0 = block_sum<kThreads>(rho, red), s1 = block_sum<kThreads>(model, red);
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = s0; part[2 * blockIdx.x + 1] = s1; }
}

// Self-check entry: one lane per case, both views free at unit Jacobi scale.  Record (22 doubles): the edge record's 21,
// then the logarithm's branch.
constexpr int kSelftestRec = 22;
__global__ __launch_bounds__(kThreads) void k_selftest_edge(int count, const double* __restrict__ w_i,
                                                            const double* __restrict__ w_j, const double* __restrict__ rel,
                                                            double b, double* __restrict__ out) {
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= count) return;
  double wi[3], wj[3], wr[3];
  const double one[3] = {1.0, 1.0, 1.0};
#pragma unroll
  for (int k = 0; k < 3; ++k) { wi[k] = w_i[3 * (size_t)e + k]; wj[k] = w_j[3 * (size_t)e + k]; wr[k] = rel[3 * (size_t)e + k]; }
  double* o = out + kSelftestRec * (size_t)e;
  int branch;
  linearise_edge(wi, wj, wr, true, true, one, one, b, o, branch);
  o[21] = (double)branch;
}

}  // namespace
}  // namespace thip

using namespace thip;

extern "C" int theia_hip_nonlinear_rotations(int32_t num_views, double* orientations, const uint8_t* fixed, int32_t num_edges,
                                             const int32_t* edges, const double* relative_rotations,
                                             const theia_nonlinear_rotation_options* options,
                                             theia_nonlinear_rotation_summary* summary, double* trace_out,
                                             int32_t trace_capacity) {
  const auto t_start = std::chrono::steady_clock::now();
  const int n = num_views, E = num_edges;
  if (!summary) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null summary");
  *summary = theia_nonlinear_rotation_summary{};
  theia_nonlinear_rotation_options o{200, 0, 0.1, 1e-6, 1e-10, 1e-8, 1e16};
  if (options) o = *options;
  // ---- refusals, before the device is touched
  if (n < 1 || !orientations) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "no views, or null orientations");
  if (E < 1 || !edges || !relative_rotations) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "no relative rotation constraints");
  if (trace_capacity < 0 || (trace_capacity > 0 && !trace_out)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "bad trace buffer");
  if (o.max_num_iterations < 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "max_num_iterations must be >= 0");
  if (!positive_finite(o.robust_loss_width)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "robust_loss_width must be positive and finite");
  if (!nonnegative_finite(o.function_tolerance) || !nonnegative_finite(o.gradient_tolerance) ||
      !nonnegative_finite(o.parameter_tolerance))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "the tolerances must be finite and not negative");
  if (!positive_finite(o.max_trust_region_radius))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "max_trust_region_radius must be positive and finite");
  std::vector<int> root;
  if (int bad = view_graph_components(n, E, edges, &root)) return bad;
  std::vector<uint8_t> out(n, 1);   // the views that take no columns: held, or without an edge
  for (int e = 0; e < E; ++e) {
    const int i = edges[2 * e], j = edges[2 * e + 1];
    if (i == j)   // Ceres refuses a residual block that names one parameter block twice
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "edge %d joins view %d to itself", e, i);
    out[i] = out[j] = 0;
  }
  for (int v = 0; v < n && fixed; ++v) if (fixed[v]) out[v] = 1;
  ViewGraphPlan g;
  fill_view_graph_lists(n, out, E, edges, &g);
  const int m = g.m;
  theia_nonlinear_rotation_summary sm{};
  sm.num_views_in_problem = m;
  if (m == 0) {   // every view of every edge is held: nothing to solve
    sm.seconds = ms_since(t_start) * 1e-3;
    *summary = sm;
    return 0;
  }
  if ((long long)m * 3 + 1 > INT32_MAX / 2) return set_error(THEIA_HIP_ERR_OUT_OF_MEMORY, "%d views: the dense system does not fit", m);
  const int n3 = 3 * m;

  int rc;
  if ((rc = thip::ensure_device())) return rc;
  hipStream_t st = nullptr;
  const int nbE = grid_of(E, kThreads), nbM = grid_of(m, kThreads), nbV = grid_of(m, kViewsPerBlock);
  const int rows = o.max_num_iterations + 1;
  DenseSpd A;   // row n3: the right-hand side
  DeviceViewGraph dg;
  DevBuf<double> d_x, d_xc, d_rel, d_rec, d_scale, d_g, d_y, d_pc, d_pg, d_pcand, d_pstep, d_trace;
  DevBuf<NlState> d_st;
  const std::vector<double> ones(n3, 1.0);
  // the dense system first: when it does not fit, that is the answer
  if ((rc = A.alloc(n3, 1)) || (rc = d_x.up(orientations, 3 * (size_t)n)) || (rc = d_xc.up(orientations, 3 * (size_t)n)) ||
      (rc = d_rel.up(relative_rotations, 3 * (size_t)E)) || (rc = dg.up(g, edges, E, n)) ||
      (rc = d_rec.alloc(kRec * (size_t)E)) || (rc = d_scale.up(ones.data(), n3)) || (rc = d_g.alloc(n3)) ||
      (rc = d_y.alloc(n3)) || (rc = d_pc.alloc(nbE)) || (rc = d_pg.alloc(nbV)) || (rc = d_pcand.alloc(2 * (size_t)nbE)) ||
      (rc = d_pstep.alloc(2 * (size_t)nbM)) || (rc = d_trace.alloc(5 * (size_t)rows)) || (rc = d_st.alloc(1)))
    return rc;
  const ViewGraphLists& vg = dg.lists;

  NlState hs{};
  lm::start(hs); hs.fresh = 1;
  HIP_TRY(hipMemcpy(d_st.p, &hs, sizeof(NlState), hipMemcpyHostToDevice));
  HIP_TRY(hipMemsetAsync(A.flag(), 0, sizeof(double), st));
  HIP_TRY(hipMemsetAsync(d_rec.p, 0, sizeof(double) * kRec * (size_t)E, st));
  const double b = o.robust_loss_width * o.robust_loss_width;
  const int* done = &d_st.p->done;

  auto linearise = [&]() {
    k_linearise<<<nbE, kThreads, 0, st>>>(E, vg.edges, vg.idx, d_x.p, d_rel.p, d_scale.p, b, d_rec.p, d_pc.p, d_st.p);
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
  const int chunk_size = lm_chunk_size();
  DecideArgs da{nbE, nbM, 3 * n, rows, THEIA_ROTATION_TERM_PARAMETER_TOLERANCE, THEIA_ROTATION_TERM_FUNCTION_TOLERANCE,
                THEIA_ROTATION_TERM_FAILURE, o.function_tolerance, o.parameter_tolerance, o.max_trust_region_radius};
  rc = run_until_done(o.max_num_iterations, chunk_size, d_st.p, &hs, [&]() {
    if (int bad = A.clear(st)) return bad;
    k_assemble<<<grid_of((size_t)m + g.P, kThreads), kThreads, 0, st>>>(vg, A.lda, d_rec.p, d_g.p, A.A(), d_st.p);
    A.factor(1, st, done);
    A.back_substitute(1, A.rhs_row(0), A.lda, d_y.p, st, done);
    k_step<<<nbM, kThreads, 0, st>>>(m, vg.free_view, d_x.p, d_scale.p, d_y.p, d_xc.p, d_pstep.p, d_st.p);
    k_candidate<<<nbE, kThreads, 0, st>>>(E, vg.edges, vg.idx, d_xc.p, d_rel.p, d_rec.p, d_y.p, b, d_pcand.p, d_st.p);
    k_decide<<<1, kThreads, 0, st>>>(da, d_pcand.p, d_pstep.p, A.flag(), d_x.p, d_xc.p, d_trace.p, d_st.p);
    linearise();
    gradient_and_post(0);
    return 0;
  });
  if (rc) return rc;
  if (!hs.done) return set_error(THEIA_HIP_ERR_INTERNAL, "the loop ended without a termination");

  // ---- Ceres copies its state back unless the solve failed
  if (hs.term != THEIA_ROTATION_TERM_FAILURE) {
    std::vector<double> x(3 * (size_t)n);
    HIP_TRY(hipMemcpy(x.data(), d_x.p, sizeof(double) * x.size(), hipMemcpyDeviceToHost));
    for (int v = 0; v < n; ++v)
      if (g.idx[v] >= 0)
        for (int c = 0; c < 3; ++c) orientations[3 * (size_t)v + c] = x[3 * (size_t)v + c];
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

extern "C" int theia_hip_selftest_pairwise_rotation_error(int32_t count, const double* w_i, const double* w_j,
                                                          const double* rel, double width, double* out) {
  if (count < 1 || count > (1 << 20)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "count = %d", count);
  if (!w_i || !w_j || !rel || !out) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null pointer");
  if (!positive_finite(width)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "width must be positive and finite");
  int rc = thip::ensure_device();
  if (rc) return rc;
  DevBuf<double> d_i, d_j, d_rel, d_out;
  const size_t n3 = 3 * (size_t)count, rec = kSelftestRec * (size_t)count;
  if ((rc = d_i.up(w_i, n3)) || (rc = d_j.up(w_j, n3)) || (rc = d_rel.up(rel, n3)) || (rc = d_out.alloc(rec))) return rc;
  k_selftest_edge<<<grid_of(count, kThreads), kThreads, 0, nullptr>>>(count, d_i.p, d_j.p, d_rel.p, width * width, d_out.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, d_out.p, sizeof(double) * rec, hipMemcpyDeviceToHost));
  return 0;
}
