// rotation_averaging.hip -- RobustRotationEstimator (global_pose_estimation/robust_rotation_estimator.{h,cc}; pybind
// sfm.cc:1749-1780): L1 ADMM regression on the view graph, then IRLS, all on the device in FP64.
//
// The reference solves with A (one 3-row block per edge: -I at view i, +I at view j, no column for a fixed view) through
// Eigen's SimplicialLDLT of the 3N x 3N matrix A'WA.  Every edge's weight is the same for its three rows, so
//   A'WA = L_w (x) I_3,   A'W e = the three columns gathered per view,
// with L_w the weighted graph Laplacian restricted to the free views: ONE N x N SPD factorisation (dense_cholesky.hip, the
// BA's K3 kernels) with three right-hand sides, 27x fewer flops than the 3N x 3N one.  The L1 stage factors L once and runs
// every ADMM solve against that factor (dense_cholesky_solve_factored); the IRLS stage assembles L_w and its three
// right-hand-side rows into one (N + 3) x lda array and factors it per iteration (forward substitution out of the panel
// steps, then dense_cholesky_back_substitute).
//
// Determinism: no atomics.  The Laplacian is assembled from host-built CSR lists (per free view: incident edges in edge
// order; per unordered free-view pair: its edges in edge order), the norms of the ADMM stopping test and the step sizes are
// block partials summed by one workgroup in block order.  Two runs on one input are bit-identical.
//
// The per-edge residual e_ij = MultiplyRotations(-r_j, MultiplyRotations(r_ij, r_i)) and the update
// r_i <- MultiplyRotations(r_i, delta_i) go through ceres' conversions (rotation_maps.h) with the intermediate angle-axis
// round trip the reference takes (math/rotation.cc:56-66).
#include "rotation_maps.h"
#include "dense_cholesky.h"
#include "view_graph_device.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

namespace thip {
namespace {

constexpr int kThreads = 256;

// ComputeResiduals (robust_rotation_estimator.cc:268-284) and the IRLS weight of every edge (:200-206):
// w = sigma / (|e|^2 + sigma^2)^2.  part[block] = sum of |e|^2 over the block's edges.
__global__ __launch_bounds__(kThreads) void k_residual(int E, const int2* __restrict__ edges, const double* __restrict__ rel,
                                                       const double* __restrict__ aa, double sigma, double* __restrict__ res,
                                                       double* __restrict__ w, double* __restrict__ part) {
  __shared__ double red[kThreads];
  const int e = blockIdx.x * kThreads + threadIdx.x;
  double sq = 0.0;
  if (e < E) {
    const int2 ij = edges[e];
    const double ri[3] = {aa[3 * ij.x], aa[3 * ij.x + 1], aa[3 * ij.x + 2]};
    const double nrj[3] = {-aa[3 * ij.y], -aa[3 * ij.y + 1], -aa[3 * ij.y + 2]};
    const double rij[3] = {rel[3 * (size_t)e], rel[3 * (size_t)e + 1], rel[3 * (size_t)e + 2]};
    double t[3], r[3];
    multiply_rotations(rij, ri, t);
    multiply_rotations(nrj, t, r);
    res[3 * (size_t)e] = r[0]; res[3 * (size_t)e + 1] = r[1]; res[3 * (size_t)e + 2] = r[2];
    sq = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
    const double tmp = sq + sigma * sigma;
    w[e] = sigma / (tmp * tmp);
  }
  const double s = block_sum<kThreads>(sq, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// The lower triangle of L_w and the rows of A'W e, into the zeroed (m + 3) x lda array:
//   thread t < m       : free view t -- diagonal sum of w over its incident edges, rhs row c = sum of sign * w * e_c
//   thread t = m + p   : pair p = (a > b) -- A[a][b] = -sum of w over the pair's edges
// vg: view_graph_device.h.  w == nullptr: unit weights (A'A, A'e).
__global__ __launch_bounds__(kThreads) void k_assemble(ViewGraphLists vg, int lda, const double* __restrict__ w,
                                                       const double* __restrict__ res, double* __restrict__ A) {
  const int t = blockIdx.x * kThreads + threadIdx.x, m = vg.m;
  if (t < m) {
    double d = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
    for (int k = vg.inc_off[t]; k < vg.inc_off[t + 1]; ++k) {
      const int e = vg.inc[k] >> 1;
      const double we = w ? w[e] : 1.0;
      const double sw = (vg.inc[k] & 1) ? we : -we;
      d += we;
      g0 += sw * res[3 * (size_t)e]; g1 += sw * res[3 * (size_t)e + 1]; g2 += sw * res[3 * (size_t)e + 2];
    }
    A[(size_t)t * lda + t] = d;
    A[(size_t)m * lda + t] = g0;
    A[(size_t)(m + 1) * lda + t] = g1;
    A[(size_t)(m + 2) * lda + t] = g2;
  } else if (t < m + vg.P) {
    const int p = t - m;
    double s = 0.0;
    for (int k = vg.pair_off[p]; k < vg.pair_off[p + 1]; ++k) s += w ? w[vg.pair_edge[k]] : 1.0;
    const int2 rc = vg.pair_rc[p];
    A[(size_t)rc.x * lda + rc.y] = -s;
  }
}

// ADMM x-update right-hand side (l1_solver.h:128): g = A' (b + z - u), [3][m].  This kernel and k_admm_view run once per
// ADMM iteration, each followed by a host read: they take the two lists they walk as pointers, which keeps their
// arguments within one 64-byte line (with the whole ViewGraphLists the L1 stage measured 0.8 % slower).
__global__ __launch_bounds__(kThreads) void k_admm_rhs(int m, const int* __restrict__ inc_off, const int* __restrict__ inc,
                                                       const double* __restrict__ b, const double* __restrict__ z,
                                                       const double* __restrict__ u, double* __restrict__ g) {
  const int v = blockIdx.x * kThreads + threadIdx.x;
  if (v >= m) return;
  double g0 = 0.0, g1 = 0.0, g2 = 0.0;
  for (int k = inc_off[v]; k < inc_off[v + 1]; ++k) {
    const size_t e3 = 3 * (size_t)(inc[k] >> 1);
    const double q0 = (b[e3] + z[e3]) - u[e3], q1 = (b[e3 + 1] + z[e3 + 1]) - u[e3 + 1], q2 = (b[e3 + 2] + z[e3 + 2]) - u[e3 + 2];
    if (inc[k] & 1) { g0 += q0; g1 += q1; g2 += q2; } else { g0 -= q0; g1 -= q1; g2 -= q2; }
  }
  g[v] = g0; g[m + v] = g1; g[2 * m + v] = g2;
}

// ADMM z / u updates of one iteration (l1_solver.h:135-145) per edge row, and the block partials of
// |A x - z - b|^2, |A x|^2, |z|^2 (:148-150) into part[block][3].
__global__ __launch_bounds__(kThreads) void k_admm_edge(int E, int m, const int2* __restrict__ edges, const int* __restrict__ idx,
                                                        const double* __restrict__ x, const double* __restrict__ b,
                                                        double* __restrict__ z, double* __restrict__ zold, double* __restrict__ u,
                                                        double alpha, double kappa, double* __restrict__ part) {
  __shared__ double red[kThreads];
  const int e = blockIdx.x * kThreads + threadIdx.x;
  double rr = 0.0, aa = 0.0, zz = 0.0;
  if (e < E) {
    const int2 ij = edges[e];
    const int a = idx[ij.x], c = idx[ij.y];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const size_t q = 3 * (size_t)e + k;
      const double xi = a >= 0 ? x[(size_t)k * m + a] : 0.0, xj = c >= 0 ? x[(size_t)k * m + c] : 0.0;
      const double ax = xj - xi;
      const double bq = b[q], zq = z[q], uq = u[q];
      const double ax_hat = alpha * ax + (1.0 - alpha) * (zq + bq);
      const double v = (ax_hat - bq) + uq;
      const double zn = soft_threshold(v, kappa);
      zold[q] = zq;
      z[q] = zn;
      u[q] = uq + ((ax_hat - zn) - bq);
      const double r = (ax - zn) - bq;
      rr += r * r; aa += ax * ax; zz += zn * zn;
    }
  }
  const double s0 = block_sum<kThreads>(rr, red), s1 = block_sum<kThreads>(aa, red), s2 = block_sum<kThreads>(zz, red);
  if (threadIdx.x == 0) { part[3 * blockIdx.x] = s0; part[3 * blockIdx.x + 1] = s1; part[3 * blockIdx.x + 2] = s2; }
}

// Dual residual and dual tolerance terms (l1_solver.h:151-156): |rho A'(z - z_old)|^2 and |rho A' u|^2, part[block][2].
__global__ __launch_bounds__(kThreads) void k_admm_view(int m, const int* __restrict__ inc_off, const int* __restrict__ inc,
                                                        const double* __restrict__ z, const double* __restrict__ zold,
                                                        const double* __restrict__ u, double rho, double* __restrict__ part) {
  __shared__ double red[kThreads];
  const int v = blockIdx.x * kThreads + threadIdx.x;
  double ss = 0.0, tt = 0.0;
  if (v < m) {
    double s[3] = {0.0, 0.0, 0.0}, t[3] = {0.0, 0.0, 0.0};
    for (int k = inc_off[v]; k < inc_off[v + 1]; ++k) {
      const size_t e3 = 3 * (size_t)(inc[k] >> 1);
      const bool plus = inc[k] & 1;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double d = z[e3 + c] - zold[e3 + c];
        s[c] += plus ? d : -d;
        t[c] += plus ? u[e3 + c] : -u[e3 + c];
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double sc = -rho * s[c], tc = rho * t[c];
      ss += sc * sc; tt += tc * tc;
    }
  }
  const double s0 = block_sum<kThreads>(ss, red), s1 = block_sum<kThreads>(tt, red);
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = s0; part[2 * blockIdx.x + 1] = s1; }
}

// UpdateGlobalRotations (:252-266): r_v <- MultiplyRotations(r_v, delta_v) for the free views, and the block partials of
// |delta_v| for ComputeAverageStepSize (:286-294).
__global__ __launch_bounds__(kThreads) void k_update(int m, const int* __restrict__ free_view, const double* __restrict__ x,
                                                     double* __restrict__ aa, double* __restrict__ part) {
  __shared__ double red[kThreads];
  const int v = blockIdx.x * kThreads + threadIdx.x;
  double step = 0.0;
  if (v < m) {
    const int id = free_view[v];
    const double d[3] = {x[v], x[(size_t)m + v], x[2 * (size_t)m + v]};
    const double r[3] = {aa[3 * (size_t)id], aa[3 * (size_t)id + 1], aa[3 * (size_t)id + 2]};
    double o[3];
    multiply_rotations(r, d, o);
    aa[3 * (size_t)id] = o[0]; aa[3 * (size_t)id + 1] = o[1]; aa[3 * (size_t)id + 2] = o[2];
    step = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
  }
  const double s = block_sum<kThreads>(step, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

}  // namespace
}  // namespace thip

using namespace thip;

extern "C" int theia_hip_robust_rotation_averaging(int32_t num_views, double* orientations, const uint8_t* fixed,
                                                   int32_t num_edges, const int32_t* edges, const double* relative_rotations,
                                                   const theia_rotation_options* o, theia_rotation_summary* summary) {
  const auto t_start = std::chrono::steady_clock::now();
  const int n = num_views, E = num_edges;
  if (n < 1 || !orientations) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "no views");
  if (E < 1 || !edges || !relative_rotations)   // CHECK_GT(relative_rotations_.size(), 0) (robust_rotation_estimator.cc:68)
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "no relative rotation constraints");
  if (!o || !summary) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null options or summary");
  if (o->max_num_l1_iterations < 0 || o->max_num_irls_iterations < 0 || !(o->irls_loss_parameter_sigma > 0.0))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "bad options");
  // every connected component needs a fixed view, else A'A is singular (the L1Solver constructor's CHECK)
  ViewGraphPlan g;
  int rc = build_view_graph_plan(n, fixed, E, edges, "fixed", &g);
  if (rc) return rc;
  *summary = theia_rotation_summary{};
  const int m = g.m;
  if (m == 0) { summary->setup_ms = ms_since(t_start); return 0; }   // nothing moves

  if ((rc = thip::ensure_device())) return rc;
  const int nbE = grid_of(E, kThreads), nbV = grid_of(m, kThreads);
  DenseSpd L;   // L_w and the three rows of A'W e
  DeviceViewGraph dg;
  DevBuf<double> d_aa, d_rel, d_res, d_w, d_b, d_z, d_u, d_zold, d_g, d_T, d_x, d_part, d_sums;
  if ((rc = L.alloc(m, 3)) || (rc = d_aa.up(orientations, 3 * (size_t)n)) || (rc = d_rel.up(relative_rotations, 3 * (size_t)E)) ||
      (rc = dg.up(g, edges, E, n)) || (rc = d_res.alloc(3 * (size_t)E)) || (rc = d_w.alloc(E)) ||
      (rc = d_b.alloc(3 * (size_t)E)) || (rc = d_z.alloc(3 * (size_t)E)) || (rc = d_u.alloc(3 * (size_t)E)) ||
      (rc = d_zold.alloc(3 * (size_t)E)) || (rc = d_g.alloc(3 * (size_t)m)) || (rc = d_T.alloc(3 * (size_t)m)) ||
      (rc = d_x.alloc(3 * (size_t)m)) || (rc = d_part.alloc(3 * (size_t)std::max(nbE, nbV))) || (rc = d_sums.alloc(8)))
    return rc;
  const ViewGraphLists& vg = dg.lists;
  hipStream_t st = nullptr;
  const double sigma = o->irls_loss_parameter_sigma;
  double sums[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  // residuals and weights of the current orientations, |e|^2 -> sums[6]
  auto residuals = [&]() {
    k_residual<<<nbE, kThreads, 0, st>>>(E, vg.edges, d_rel.p, d_aa.p, sigma, d_res.p, d_w.p, d_part.p);
    k_sum_partials<kThreads><<<1, kThreads, 0, st>>>(d_part.p, nbE, 1, d_sums.p + 6);
  };
  // update with d_x, new residuals; returns the average step size (sums[5] / m)
  auto update = [&](double* avg) -> int {
    k_update<<<nbV, kThreads, 0, st>>>(m, vg.free_view, d_x.p, d_aa.p, d_part.p);
    k_sum_partials<kThreads><<<1, kThreads, 0, st>>>(d_part.p, nbV, 1, d_sums.p + 5);
    residuals();
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(sums, d_sums.p, sizeof(sums), hipMemcpyDeviceToHost));
    *avg = sums[5] / m;
    return 0;
  };
  auto give_back = [&]() -> int {
    HIP_TRY(hipMemcpy(orientations, d_aa.p, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToHost));
    return 0;
  };

  // ---- L1 stage (SolveL1Regression, :164-185; L1Solver, math/l1_solver.h): factor A'A = L (x) I_3 once
  if ((rc = L.clear(st, true))) return rc;
  HIP_TRY(hipMemsetAsync(d_x.p, 0, sizeof(double) * 3 * m, st));
  residuals();
  k_assemble<<<grid_of(m + g.P, kThreads), kThreads, 0, st>>>(vg, L.lda, nullptr, d_res.p, L.A());
  L.factor(1, st);   // row m (A'e, unused) rides along
  bool failed = false;
  if ((rc = L.failed(&failed))) return rc;
  HIP_TRY(hipMemcpy(sums, d_sums.p, sizeof(sums), hipMemcpyDeviceToHost));
  summary->setup_ms = ms_since(t_start);
  if (failed) return set_error(THEIA_HIP_ERR_INTERNAL, "the Cholesky factorisation of A'A failed");
  const auto t_l1 = std::chrono::steady_clock::now();
  const double rho = 1.0, alpha = 1.0, abs_tol = 1e-4, rel_tol = 1e-2;
  const double primal_abs_eps = std::sqrt(3.0 * E) * abs_tol, dual_abs_eps = std::sqrt(3.0 * m) * abs_tol;
  int max_admm = 5;
  for (int pass = 0; pass < o->max_num_l1_iterations; ++pass) {
    // L1Solver::Solve(residual, &step): z = u = 0, b = residual
    HIP_TRY(hipMemcpyAsync(d_b.p, d_res.p, sizeof(double) * 3 * E, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemsetAsync(d_z.p, 0, sizeof(double) * 3 * E, st));
    HIP_TRY(hipMemsetAsync(d_u.p, 0, sizeof(double) * 3 * E, st));
    const double rhs_norm = std::sqrt(sums[6]);
    for (int it = 0; it < max_admm; ++it) {
      k_admm_rhs<<<nbV, kThreads, 0, st>>>(m, vg.inc_off, vg.inc, d_b.p, d_z.p, d_u.p, d_g.p);
      L.solve_factored(3, d_g.p, d_T.p, d_x.p, st);
      k_admm_edge<<<nbE, kThreads, 0, st>>>(E, m, vg.edges, vg.idx, d_x.p, d_b.p, d_z.p, d_zold.p, d_u.p, alpha, 1.0 / rho, d_part.p);
      k_sum_partials<kThreads><<<1, kThreads, 0, st>>>(d_part.p, nbE, 3, d_sums.p);
      k_admm_view<<<nbV, kThreads, 0, st>>>(m, vg.inc_off, vg.inc, d_z.p, d_zold.p, d_u.p, rho, d_part.p);
      k_sum_partials<kThreads><<<1, kThreads, 0, st>>>(d_part.p, nbV, 2, d_sums.p + 3);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpy(sums, d_sums.p, sizeof(double) * 5, hipMemcpyDeviceToHost));
      ++summary->admm_iterations;
      const double r_norm = std::sqrt(sums[0]), s_norm = std::sqrt(sums[3]);
      const double max_norm = std::max({std::sqrt(sums[1]), std::sqrt(sums[2]), rhs_norm});
      const double primal_eps = primal_abs_eps + rel_tol * max_norm;
      const double dual_eps = dual_abs_eps + rel_tol * std::sqrt(sums[4]);
      if (r_norm < primal_eps && s_norm < dual_eps) break;
    }
    double avg = 0.0;
    if ((rc = update(&avg))) return rc;
    ++summary->l1_iterations;
    if (avg <= o->l1_step_convergence_threshold) break;
    max_admm *= 2;
  }
  summary->l1_ms = ms_since(t_l1);

  // ---- IRLS stage (SolveIRLS, :187-250): per iteration factor L_w with the three rows of A'W e forward-substituted
  const auto t_irls = std::chrono::steady_clock::now();
  for (int it = 0; it < o->max_num_irls_iterations; ++it) {
    if ((rc = L.clear(st))) return rc;
    k_assemble<<<grid_of(m + g.P, kThreads), kThreads, 0, st>>>(vg, L.lda, d_w.p, d_res.p, L.A());
    L.factor(3, st);
    if ((rc = L.failed(&failed))) return rc;
    if (failed) {
      summary->irls_ms = ms_since(t_irls);
      summary->final_squared_residual = sums[6];
      if ((rc = give_back())) return rc;
      return set_error(THEIA_HIP_ERR_INTERNAL, "the Cholesky factorisation of A'WA failed in IRLS iteration %d", it);
    }
    L.back_substitute(3, L.rhs_row(0), L.lda, d_x.p, st);
    double avg = 0.0;
    if ((rc = update(&avg))) return rc;
    ++summary->irls_iterations;
    if (avg < o->irls_step_convergence_threshold) break;
  }
  summary->irls_ms = ms_since(t_irls);
  summary->final_squared_residual = sums[6];
  return give_back();
}
