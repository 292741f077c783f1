// lud_positions.hip -- LeastUnsquaredDeviationPositionEstimator (global_pose_estimation/
// least_unsquared_deviation_position_estimator.cc:75-213; pybind sfm.cc:1707-1726): the constrained L1 ADMM of
// ConstrainedL1Solver (math/constrained_l1_solver.cc:49-187) on the device in FP64.
//
// The reference stacks, per view pair e = (i, j), three rows c_j - c_i - s_e d_e (d_e = R_i' position_2) and one row s_e
// against the bound 1 into A, with unknowns x = [3 (N-1) positions | one scale per pair], and factors A'A once with a
// sparse LLT.  Each scale column touches only its pair's four rows, so the scale block of A'A is diagonal,
// D_e = |d_e|^2 + 1, and eliminating the scales leaves the SPD matrix-weighted Laplacian of order 3m (m free views)
//   S = sum_e K_e (x) M_e,   M_e = I_3 - d_e d_e' / D_e,   K_e = [[1, -1], [-1, 1]] on (i, j).
// S is factored once (dense_cholesky.hip, the BA's K3 kernels); every ADMM x-update is
//   reduced rhs   r_v = sum over incident edges of -/+ (w_e + d_e g_s,e / D_e),  w = b + z - u,  g_s,e = w_q,e - d_e . w_e
//   solve         S x_p = r                   (dense_cholesky_solve_factored, k = 1)
//   scales        s_e = (g_s,e - d_e . (x_i - x_j)) / D_e
// the same system the reference solves, rounded differently.
//
// Stopping test on the device: k_test evaluates the reference's test (:150-168) from the reduced sums in one workgroup,
// counts the iteration and raises `done` when the test passes; every ADMM kernel (the solve's included) returns at once
// while `done` is set.  The host enqueues the iterations in chunks and reads the flag once per chunk, so the iteration
// count and the iterate are those of a test after every iteration, without a host round trip per iteration.
//
// Determinism: no atomics.  S is assembled from host-built CSR lists (per free view: incident edges in edge order; per
// unordered free-view pair: its edges in edge order); a free view's sums over its edges are strided over a wavefront's
// lanes and added by the butterfly; every norm is a per-block sum followed by one workgroup summing the blocks in order.
// Two runs on one input are bit-identical.
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
static_assert(kThreads == 64 * kViewsPerBlock, "k_rhs, k_view: one wavefront per free view");
constexpr int kChunk = 32;   // ADMM iterations enqueued between two reads of the `done` flag

// Device-side state of the stopping test.
struct LudState {
  int done, iterations, pad0, pad1;
  double r_norm, s_norm, primal_eps, dual_eps;
};

// GetRotatedTranslation (:63-70): d_e = R_i' position_2 (ceres angle-axis -> matrix), and D_e = |d_e|^2 + 1.
__global__ __launch_bounds__(kThreads) void k_setup(int E, const int2* __restrict__ edges, const double* __restrict__ aa,
                                                    const double* __restrict__ rel, double* __restrict__ d,
                                                    double* __restrict__ D) {
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= E) return;
  const int i = edges[e].x;
  double R[9];
  rsc::angle_axis_to_rot(aa + 3 * (size_t)i, R);
  const double t0 = rel[3 * (size_t)e], t1 = rel[3 * (size_t)e + 1], t2 = rel[3 * (size_t)e + 2];
  double dd[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) dd[c] = (R[c] * t0 + R[3 + c] * t1) + R[6 + c] * t2;
  d[3 * (size_t)e] = dd[0]; d[3 * (size_t)e + 1] = dd[1]; d[3 * (size_t)e + 2] = dd[2];
  D[e] = ((dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2]) + 1.0;
}

__device__ __forceinline__ double m_entry(const double* d, double De, int r, int c) {
  return (r == c ? 1.0 : 0.0) - (d[r] * d[c]) / De;
}

// The lower triangle of S into the zeroed array (row-major, leading dimension lda):
//   thread t < m       : free view t -- its 3 x 3 diagonal block, sum of M_e over its incident edges
//   thread t = m + p   : pair p = (a > b) -- block (a, b) = -sum of M_e over the pair's edges
// vg: view_graph_device.h.
__global__ __launch_bounds__(kThreads) void k_assemble(ViewGraphLists vg, int lda, const double* __restrict__ d,
                                                       const double* __restrict__ D, double* __restrict__ S) {
  const int t = blockIdx.x * kThreads + threadIdx.x, m = vg.m;
  double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (t < m) {
    for (int k = vg.inc_off[t]; k < vg.inc_off[t + 1]; ++k) {
      const int e = vg.inc[k] >> 1;
      const double de[3] = {d[3 * (size_t)e], d[3 * (size_t)e + 1], d[3 * (size_t)e + 2]};
      const double De = D[e];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) acc[3 * r + c] += m_entry(de, De, r, c);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c <= r; ++c) S[(size_t)(3 * t + r) * lda + 3 * t + c] = acc[3 * r + c];
  } else if (t < m + vg.P) {
    const int p = t - m;
    for (int k = vg.pair_off[p]; k < vg.pair_off[p + 1]; ++k) {
      const int e = vg.pair_edge[k];
      const double de[3] = {d[3 * (size_t)e], d[3 * (size_t)e + 1], d[3 * (size_t)e + 2]};
      const double De = D[e];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[3 * r + c] += m_entry(de, De, r, c);
    }
    const int2 rc = vg.pair_rc[p];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) S[(size_t)(3 * rc.x + r) * lda + 3 * rc.y + c] = -acc[3 * r + c];
  }
}

// w = b + z - u of one edge's four rows (b = 0 on the three L1 rows, 1 on the inequality row) and the scale's
// right-hand side g_s = w_q - d . w_p.
__device__ __forceinline__ double edge_w(const double* __restrict__ z, const double* __restrict__ u, size_t e4,
                                         const double* de, double* w) {
  w[0] = z[e4] - u[e4]; w[1] = z[e4 + 1] - u[e4 + 1]; w[2] = z[e4 + 2] - u[e4 + 2];
  w[3] = (1.0 + z[e4 + 3]) - u[e4 + 3];
  return w[3] - ((de[0] * w[0] + de[1] * w[1]) + de[2] * w[2]);
}

// Reduced right-hand side of the x-update (:145): g_v = sum over incident edges of -/+ (w_e + d_e g_s,e / D_e), view-major.
// One wavefront per free view (for_each_incident_edge), then the butterfly sums the lanes in a fixed order.
__global__ __launch_bounds__(kThreads) void k_rhs(ViewGraphLists vg, const double* __restrict__ d, const double* __restrict__ D,
                                                  const double* __restrict__ z, const double* __restrict__ u,
                                                  double* __restrict__ g, const LudState* __restrict__ st) {
  if (st->done) return;
  const int v = blockIdx.x * kViewsPerBlock + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (v >= vg.m) return;   // wave-uniform
  double g0 = 0.0, g1 = 0.0, g2 = 0.0;
  for_each_incident_edge(vg, v, lane, [&](int e, bool plus) {
    const double de[3] = {d[3 * (size_t)e], d[3 * (size_t)e + 1], d[3 * (size_t)e + 2]};
    double w[4];
    const double f = edge_w(z, u, 4 * (size_t)e, de, w) / D[e];
    const double h0 = w[0] + de[0] * f, h1 = w[1] + de[1] * f, h2 = w[2] + de[2] * f;
    if (plus) { g0 += h0; g1 += h1; g2 += h2; } else { g0 -= h0; g1 -= h1; g2 -= h2; }
  });
  g0 = wave_sum_butterfly(g0); g1 = wave_sum_butterfly(g1); g2 = wave_sum_butterfly(g2);
  if (lane == 0) { g[3 * (size_t)v] = g0; g[3 * (size_t)v + 1] = g1; g[3 * (size_t)v + 2] = g2; }
}

// After the solve, per edge (:146-160): the scale back-substitution, A x, over-relaxation, ModifiedShrinkage, the u
// update, z - z_old, and the block partials of |Ax - z - b|^2, |Ax|^2, |z|^2 and of the scale rows' terms of
// |rho A'(z - z_old)|^2 and |rho A'u|^2, into part[block][5].
__global__ __launch_bounds__(kThreads) void k_edge(int E, const int2* __restrict__ edges, const int* __restrict__ idx,
                                                   const double* __restrict__ d, const double* __restrict__ D,
                                                   const double* __restrict__ x, double* __restrict__ z,
                                                   double* __restrict__ u, double* __restrict__ dz, double alpha,
                                                   double kappa, double rho, double* __restrict__ part,
                                                   const LudState* __restrict__ st) {
  __shared__ double red[kThreads];
  if (st->done) return;
  const int e = blockIdx.x * kThreads + threadIdx.x;
  double rr = 0.0, aa = 0.0, zz = 0.0, ss = 0.0, tt = 0.0;
  if (e < E) {
    const int2 ij = edges[e];
    const int a = idx[ij.x], c = idx[ij.y];
    const double de[3] = {d[3 * (size_t)e], d[3 * (size_t)e + 1], d[3 * (size_t)e + 2]};
    const size_t e4 = 4 * (size_t)e;
    double w[4];
    const double gs = edge_w(z, u, e4, de, w);
    double xi[3], xj[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      xi[k] = a >= 0 ? x[3 * (size_t)a + k] : 0.0;
      xj[k] = c >= 0 ? x[3 * (size_t)c + k] : 0.0;
    }
    const double s = (gs - ((de[0] * (xi[0] - xj[0]) + de[1] * (xi[1] - xj[1])) + de[2] * (xi[2] - xj[2]))) / D[e];
    double ax[4];
#pragma unroll
    for (int k = 0; k < 3; ++k) ax[k] = (xj[k] - xi[k]) - s * de[k];
    ax[3] = s;
    double dzn[4], un[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double bq = q == 3 ? 1.0 : 0.0, zq = z[e4 + q], uq = u[e4 + q];
      const double ax_hat = alpha * ax[q] + (1.0 - alpha) * (zq + bq);
      const double v = (ax_hat - bq) + uq;
      const double zn = q == 3 ? fmax(v, 0.0) : soft_threshold(v, kappa);
      un[q] = uq + ((ax_hat - zn) - bq);
      dzn[q] = zn - zq;
      z[e4 + q] = zn;
      u[e4 + q] = un[q];
      dz[e4 + q] = dzn[q];
      const double r = (ax[q] - zn) - bq;
      rr += r * r; aa += ax[q] * ax[q]; zz += zn * zn;
    }
    const double sc = rho * (dzn[3] - ((de[0] * dzn[0] + de[1] * dzn[1]) + de[2] * dzn[2]));
    const double tc = rho * (un[3] - ((de[0] * un[0] + de[1] * un[1]) + de[2] * un[2]));
    ss = sc * sc; tt = tc * tc;
  }
  const double s0 = block_sum<kThreads>(rr, red), s1 = block_sum<kThreads>(aa, red), s2 = block_sum<kThreads>(zz, red);
  const double s3 = block_sum<kThreads>(ss, red), s4 = block_sum<kThreads>(tt, red);
  if (threadIdx.x == 0) {
    double* p = part + 5 * (size_t)blockIdx.x;
    p[0] = s0; p[1] = s1; p[2] = s2; p[3] = s3; p[4] = s4;
  }
}

// The position rows of |rho A'(z - z_old)|^2 and |rho A'u|^2 (:157, :162), one wavefront per free view as in k_rhs;
// part[block][2] = the sums of the workgroup's views in view order.
__global__ __launch_bounds__(kThreads) void k_view(ViewGraphLists vg, const double* __restrict__ dz,
                                                   const double* __restrict__ u, double rho, double* __restrict__ part,
                                                   const LudState* __restrict__ st) {
  __shared__ double red[2][kViewsPerBlock];
  if (st->done) return;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int v = blockIdx.x * kViewsPerBlock + wv;
  double ss = 0.0, tt = 0.0;
  if (v < vg.m) {   // wave-uniform
    double s[3] = {0.0, 0.0, 0.0}, t[3] = {0.0, 0.0, 0.0};
    for_each_incident_edge(vg, v, lane, [&](int e, bool plus) {
      const size_t e4 = 4 * (size_t)e;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        s[c] += plus ? dz[e4 + c] : -dz[e4 + c];
        t[c] += plus ? u[e4 + c] : -u[e4 + c];
      }
    });
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double sc = rho * wave_sum_butterfly(s[c]), tc = rho * wave_sum_butterfly(t[c]);
      ss += sc * sc; tt += tc * tc;
    }
  }
  if (lane == 0) { red[0][wv] = ss; red[1][wv] = tt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, b = 0.0;
    for (int k = 0; k < kViewsPerBlock; ++k) { a += red[0][k]; b += red[1][k]; }
    part[2 * blockIdx.x] = a; part[2 * blockIdx.x + 1] = b;
  }
}

// One workgroup: sums the blocks' partials in block order, then thread 0 runs the reference's stopping test (:150-168),
// counts the iteration and raises `done` when it passes.
__global__ __launch_bounds__(kThreads) void k_test(const double* __restrict__ part_e, int nbE,
                                                   const double* __restrict__ part_v, int nbV, double rhs_norm,
                                                   double primal_abs_eps, double dual_abs_eps, double rel_tol,
                                                   LudState* __restrict__ st) {
  __shared__ double red[kThreads];
  if (st->done) return;
  double sum[7];
  for (int c = 0; c < 5; ++c) sum[c] = block_sum_column<kThreads>(part_e, nbE, 5, c, red);
  for (int c = 0; c < 2; ++c) sum[5 + c] = block_sum_column<kThreads>(part_v, nbV, 2, c, red);
  if (threadIdx.x == 0) {
    const double r_norm = sqrt(sum[0]);
    const double s_norm = sqrt(sum[5] + sum[3]);
    const double max_norm = fmax(fmax(sqrt(sum[1]), sqrt(sum[2])), rhs_norm);
    const double primal_eps = primal_abs_eps + rel_tol * max_norm;
    const double dual_eps = dual_abs_eps + rel_tol * sqrt(sum[6] + sum[4]);
    st->iterations += 1;
    st->r_norm = r_norm; st->s_norm = s_norm; st->primal_eps = primal_eps; st->dual_eps = dual_eps;
    if (r_norm < primal_eps && s_norm < dual_eps) st->done = 1;
  }
}

}  // namespace
}  // namespace thip

using namespace thip;

extern "C" int theia_hip_lud_positions(int32_t num_views, const double* orientations, const uint8_t* fixed,
                                       int32_t num_edges, const int32_t* edges, const double* relative_translations,
                                       const theia_lud_options* o, double* positions_out, theia_lud_summary* summary) {
  const auto t_start = std::chrono::steady_clock::now();
  const int n = num_views, E = num_edges;
  if (n < 1 || !orientations || !positions_out) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "no views");
  if (E < 1 || !edges || !relative_translations)   // an empty system: the reference's CHECK on the factorisation
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "no view pairs");
  if (!o || !summary) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null options or summary");
  if (o->max_num_iterations <= 0 || !(o->rho > 0.0) || !std::isfinite(o->rho) || !std::isfinite(o->alpha) ||
      !std::isfinite(o->absolute_tolerance) || !std::isfinite(o->relative_tolerance))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "bad options");
  // every connected component needs a held view, else S (and the reference's A'A) is singular
  ViewGraphPlan g;
  int rc = build_view_graph_plan(n, fixed, E, edges, "held", &g);
  if (rc) return rc;
  const int m = g.m, n3 = 3 * m;

  if ((rc = thip::ensure_device())) return rc;
  const int nbE = grid_of(E, kThreads), nbV = std::max(1, (m + kViewsPerBlock - 1) / kViewsPerBlock);
  DenseSpd S;   // row n3: the factorisation's right-hand-side row (zero, unused)
  DeviceViewGraph dg;
  DevBuf<double> d_aa, d_rel, d_d, d_D, d_z, d_u, d_dz, d_g, d_T, d_x, d_pe, d_pv;
  DevBuf<LudState> d_st;
  if ((rc = S.alloc(n3, 1)) || (rc = d_aa.up(orientations, 3 * (size_t)n)) ||
      (rc = d_rel.up(relative_translations, 3 * (size_t)E)) || (rc = dg.up(g, edges, E, n)) ||
      (rc = d_d.alloc(3 * (size_t)E)) || (rc = d_D.alloc(E)) || (rc = d_z.alloc(4 * (size_t)E)) ||
      (rc = d_u.alloc(4 * (size_t)E)) || (rc = d_dz.alloc(4 * (size_t)E)) || (rc = d_g.alloc(n3)) ||
      (rc = d_T.alloc(n3)) || (rc = d_x.alloc(n3)) || (rc = d_pe.alloc(5 * (size_t)nbE)) ||
      (rc = d_pv.alloc(2 * (size_t)nbV)) || (rc = d_st.alloc(1)))
    return rc;
  const ViewGraphLists& vg = dg.lists;
  theia_lud_summary sm{};
  hipStream_t st = nullptr;

  // ---- setup: d_e, D_e, S (ConstrainedL1Solver's constructor, :49-91, in Schur form)
  if ((rc = S.clear(st, true))) return rc;
  HIP_TRY(hipMemsetAsync(d_x.p, 0, sizeof(double) * std::max(1, n3), st));
  HIP_TRY(hipMemsetAsync(d_z.p, 0, sizeof(double) * 4 * (size_t)E, st));
  HIP_TRY(hipMemsetAsync(d_u.p, 0, sizeof(double) * 4 * (size_t)E, st));
  HIP_TRY(hipMemsetAsync(d_st.p, 0, sizeof(LudState), st));
  k_setup<<<nbE, kThreads, 0, st>>>(E, vg.edges, d_aa.p, d_rel.p, d_d.p, d_D.p);
  k_assemble<<<grid_of(m + g.P, kThreads), kThreads, 0, st>>>(vg, S.lda, d_d.p, d_D.p, S.A());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  sm.setup_ms = ms_since(t_start);

  // ---- factor S once
  const auto t_factor = std::chrono::steady_clock::now();
  S.factor(1, st);
  bool failed = false;
  if ((rc = S.failed(&failed))) return rc;
  sm.factor_ms = ms_since(t_factor);
  if (failed) {
    *summary = sm;
    return set_error(THEIA_HIP_ERR_INTERNAL, "the Cholesky factorisation of the reduced system failed");
  }

  // ---- ADMM (ConstrainedL1Solver::Solve, :111-170): A has 4E rows and 3m + E columns, b = [0; 1]
  const auto t_admm = std::chrono::steady_clock::now();
  const double rhs_norm = std::sqrt((double)E);
  const double primal_abs_eps = std::sqrt(4.0 * E) * o->absolute_tolerance;
  const double dual_abs_eps = std::sqrt((double)n3 + E) * o->absolute_tolerance;
  const double kappa = 1.0 / o->rho;
  const int* done = &d_st.p->done;
  LudState hs{};
  rc = run_until_done(o->max_num_iterations, kChunk, d_st.p, &hs, [&]() {
    k_rhs<<<nbV, kThreads, 0, st>>>(vg, d_d.p, d_D.p, d_z.p, d_u.p, d_g.p, d_st.p);
    S.solve_factored(1, d_g.p, d_T.p, d_x.p, st, done);
    k_edge<<<nbE, kThreads, 0, st>>>(E, vg.edges, vg.idx, d_d.p, d_D.p, d_x.p, d_z.p, d_u.p, d_dz.p, o->alpha, kappa, o->rho,
                                     d_pe.p, d_st.p);
    k_view<<<nbV, kThreads, 0, st>>>(vg, d_dz.p, d_u.p, o->rho, d_pv.p, d_st.p);
    k_test<<<1, kThreads, 0, st>>>(d_pe.p, nbE, d_pv.p, nbV, rhs_norm, primal_abs_eps, dual_abs_eps, o->relative_tolerance,
                                   d_st.p);
    return 0;
  });
  if (rc) return rc;
  std::vector<double> x(std::max(1, n3));
  HIP_TRY(hipMemcpy(x.data(), d_x.p, sizeof(double) * std::max(1, n3), hipMemcpyDeviceToHost));
  sm.admm_ms = ms_since(t_admm);
  sm.admm_iterations = hs.iterations;
  sm.converged = hs.done;
  sm.r_norm = hs.r_norm; sm.s_norm = hs.s_norm; sm.primal_eps = hs.primal_eps; sm.dual_eps = hs.dual_eps;
  for (int v = 0; v < n; ++v)
    for (int c = 0; c < 3; ++c) positions_out[3 * (size_t)v + c] = g.idx[v] >= 0 ? x[3 * (size_t)g.idx[v] + c] : 0.0;
  *summary = sm;
  return 0;
}
