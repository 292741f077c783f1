// linear_rotations.hip -- LinearRotationEstimator (global_pose_estimation/linear_rotation_estimator.{h,cc}; Martinec &
// Pajdla, "Robust Rotation and Translation Estimation in Multiview Reconstruction"): global orientations from the pairs'
// relative rotations alone, without an initial guess, on the device in FP64.
//
// Per pair e = (i, j) with R_e = AngleAxisToRotationMatrix(rotation_2), R_j = R_e R_i, the 3n x 3n symmetric matrix M
// (n = the views that have an edge) gets +I on the diagonal blocks (i, i) and (j, j), -R_e' at block (i, j) and -R_e at
// block (j, i) (linear_rotation_estimator.cc:90-150; the reference keeps the upper block only).  The three eigenvectors of
// the smallest eigenvalues, stacked as X [3n][3], hold X_i = R_i Q / sqrt(n) for one common orthogonal Q, and a view's
// orientation is ProjectToRotationMatrix(X_i) (:170-201, sfm/pose/util.cc:117-129).
//
// Stages:
//   plan (host)       the views with edges indexed compactly in view order, and per 3 x 3 block of the lower triangle the
//                     list of its edges in edge order (view_graph_plan.h, no view fixed)
//   k_rel_matrices    one thread per edge: R_e
//   k_lin_assemble    one thread per view: degree * I (an integer count, exact); one thread per lower pair block (a, b),
//                     a > b: -sum R_e over its edges (b -> a) and -sum R_e' over its edges (a -> b), added in edge order
//   k_shift           mu = 3n eps max diag M on the diagonal (spectral_shift.h)
//   dense_cholesky_factor once
//   k_start_block     X0[r][k] = (((uint32)((3 r + k + 1) * 2654435761u)) >> 8) * 2^-23 - 1, orthonormalised.  Not the stacked
//                     identities: a ring of cameras has a singular mean rotation, and that start would be orthogonal to a
//                     part of the solution
//   per iteration     dense_cholesky_solve_factored with three vectors, Y = (M + mu I)^-1 X, then k_subspace_step (one
//                     workgroup): Q = Y orthonormalised by modified Gram-Schmidt in column order, two passes;
//                     d = |Q - X (X' Q)|_F; H = X' Y; the stop flag when d <= threshold.  Every later launch of a chunk
//                     tests the flag first, and the host reads it once per chunk (the pattern of ligt_positions.hip)
//   k_project_so3     one thread per view: the Jacobi SVD of its block, U V', negated when the determinant is negative,
//                     RotationMatrixToAngleAxis
// Only the invariant subspace matters to the result: there is no Rayleigh-Ritz rotation of the vectors, and the common
// rotation Q is whatever the iteration arrives at (the reference fixes no view either).
//
// Determinism: no floating-point atomics.  Every entry of M is a sum in edge order by one owner, every dot product and norm
// a fixed tree (block_sum).  Two runs on one input are bit-identical.
#include "small_linalg.h"
#include "rotation_maps.h"
#include "dense_cholesky.h"
#include "spectral_shift.h"
#include "view_graph_device.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

namespace thip {
namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 4;   // iterations enqueued between two reads of the `done` flag

struct LinearState {
  int done, converged, iterations, pad;
  double change, shift, max_diag;
  double H[9];   // X' Y of the last step, row-major
};

__global__ __launch_bounds__(kThreads) void k_rel_matrices(int E, const double* __restrict__ rel, double* __restrict__ R) {
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= E) return;
  double r[9];
  rsc::angle_axis_to_rot(rel + 3 * (size_t)e, r);
#pragma unroll
  for (int k = 0; k < 9; ++k) R[9 * (size_t)e + k] = r[k];
}

// The lower triangle of M into the zeroed array.  Thread t < m: view t's diagonal, its degree.  Thread t = m + p: pair
// p = (a, b), a > b: block (a, b) = -sum over the pair's edges of R_e (the edge runs b -> a) or R_e' (a -> b).
// vg: view_graph_device.h; vg.idx: view -> index in the system.
__global__ __launch_bounds__(kThreads) void k_lin_assemble(ViewGraphLists vg, int lda, const double* __restrict__ R,
                                                           double* __restrict__ M) {
  const int t = blockIdx.x * kThreads + threadIdx.x, m = vg.m;
  if (t < m) {
    const double degree = (double)(vg.inc_off[t + 1] - vg.inc_off[t]);
#pragma unroll
    for (int r = 0; r < 3; ++r) M[(size_t)(3 * t + r) * lda + 3 * t + r] = degree;
  } else if (t < m + vg.P) {
    const int p = t - m;
    const int2 rc = vg.pair_rc[p];
    double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = vg.pair_off[p]; k < vg.pair_off[p + 1]; ++k) {
      const int e = vg.pair_edge[k];
      const double* v = R + 9 * (size_t)e;
      if (vg.idx[vg.edges[e].y] == rc.x) {
#pragma unroll
        for (int q = 0; q < 9; ++q) acc[q] += v[q];
      } else {
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[3 * r + c] += v[3 * c + r];
      }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) M[(size_t)(3 * rc.x + r) * lda + 3 * rc.y + c] = -acc[3 * r + c];
  }
}

// Modified Gram-Schmidt over the three vectors Q[k][n] in column order, two passes; every thread owns the rows
// threadIdx.x, threadIdx.x + kThreads, ...  False when a norm is zero or not finite (Q is then partly updated).
__device__ __forceinline__ bool orthonormalise3(int n, double* __restrict__ Q, double* red) {
  for (int pass = 0; pass < 2; ++pass)
    for (int k = 0; k < 3; ++k) {
      double* qk = Q + (size_t)k * n;
      for (int j = 0; j < k; ++j) {
        const double* qj = Q + (size_t)j * n;
        double s = 0.0;
        for (int r = threadIdx.x; r < n; r += kThreads) s += qj[r] * qk[r];
        const double c = block_sum<kThreads>(s, red);
        for (int r = threadIdx.x; r < n; r += kThreads) qk[r] -= c * qj[r];
      }
      double s = 0.0;
      for (int r = threadIdx.x; r < n; r += kThreads) s += qk[r] * qk[r];
      const double norm = sqrt(block_sum<kThreads>(s, red));
      if (!(norm > 0.0) || !isfinite(norm)) return false;   // the same in every thread
      for (int r = threadIdx.x; r < n; r += kThreads) qk[r] /= norm;
    }
  return true;
}

// out[3 j + k] = A_j . B_k over the n rows, in every thread
__device__ __forceinline__ void gram3(int n, const double* __restrict__ A, const double* __restrict__ B, double* out,
                                      double* red) {
  for (int j = 0; j < 3; ++j)
    for (int k = 0; k < 3; ++k) {
      double s = 0.0;
      for (int r = threadIdx.x; r < n; r += kThreads) s += A[(size_t)j * n + r] * B[(size_t)k * n + r];
      out[3 * j + k] = block_sum<kThreads>(s, red);
    }
}

// One workgroup: the start block into x [3][n] and, as the first right-hand side, into b.
__global__ __launch_bounds__(kThreads) void k_start_block(int n, double* __restrict__ x, double* __restrict__ b) {
  __shared__ double red[kThreads];
  for (int k = 0; k < 3; ++k)
    for (int r = threadIdx.x; r < n; r += kThreads) {
      const unsigned h = (3u * (unsigned)r + (unsigned)k + 1u) * 2654435761u;
      x[(size_t)k * n + r] = (double)(h >> 8) * 0x1p-23 - 1.0;
    }
  orthonormalise3(n, x, red);   // the hashed columns are far from dependent: no breakdown to report
  for (int k = 0; k < 3; ++k)
    for (int r = threadIdx.x; r < n; r += kThreads) b[(size_t)k * n + r] = x[(size_t)k * n + r];
}

// One workgroup, after y = (M + mu I)^-1 x (three vectors of n rows, the solve has consumed b): Q = y orthonormalised,
// built in b, which is the next right-hand side; d = |Q - x (x' Q)|_F; H = x' y; x = Q; the count and the stop flag.
__global__ __launch_bounds__(kThreads) void k_subspace_step(int n, const double* __restrict__ y, double* __restrict__ x,
                                                            double* __restrict__ b, double threshold,
                                                            LinearState* __restrict__ st) {
  __shared__ double red[kThreads];
  if (st->done) return;
  for (int k = 0; k < 3; ++k)
    for (int r = threadIdx.x; r < n; r += kThreads) b[(size_t)k * n + r] = y[(size_t)k * n + r];
  if (!orthonormalise3(n, b, red)) {   // a breakdown of the solve: stop, not converged, x stays
    if (threadIdx.x == 0) { st->iterations += 1; st->done = 1; st->converged = 0; st->change = INFINITY; }
    return;
  }
  double G[9], H[9];
  gram3(n, x, b, G, red);
  double dd = 0.0;
  for (int r = threadIdx.x; r < n; r += kThreads) {
    const double x0 = x[r], x1 = x[(size_t)n + r], x2 = x[2 * (size_t)n + r];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double d = b[(size_t)k * n + r] - ((x0 * G[k] + x1 * G[3 + k]) + x2 * G[6 + k]);
      dd += d * d;
    }
  }
  const double change = sqrt(block_sum<kThreads>(dd, red));
  gram3(n, x, y, H, red);
  for (int k = 0; k < 3; ++k)
    for (int r = threadIdx.x; r < n; r += kThreads) x[(size_t)k * n + r] = b[(size_t)k * n + r];
  if (threadIdx.x == 0) {
    st->iterations += 1;
    st->change = change;
#pragma unroll
    for (int q = 0; q < 9; ++q) st->H[q] = H[q];
    if (change <= threshold) { st->done = 1; st->converged = 1; }
  }
}

// ProjectToRotationMatrix (sfm/pose/util.cc:117-129) of view v's block X_v[r][k] = x[k][3 v + r], as angle-axis.
__global__ __launch_bounds__(kThreads) void k_project_so3(int m, int n, const double* __restrict__ x, double* __restrict__ aa) {
  const int v = blockIdx.x * kThreads + threadIdx.x;
  if (v >= m) return;
  double A[9], U[9], S[3], V[9], Rm[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) A[3 * r + k] = x[(size_t)k * n + 3 * v + r];
  rsc::svd_sq<3>(A, U, S, V);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) Rm[3 * r + c] = (U[3 * r] * V[3 * c] + U[3 * r + 1] * V[3 * c + 1]) + U[3 * r + 2] * V[3 * c + 2];
  if (rsc::det3(Rm) < 0.0) {
#pragma unroll
    for (int q = 0; q < 9; ++q) Rm[q] = -Rm[q];
  }
  double o[3];
  rsc::rot_to_angle_axis(Rm, o);
  aa[3 * (size_t)v] = o[0]; aa[3 * (size_t)v + 1] = o[1]; aa[3 * (size_t)v + 2] = o[2];
}

// eigenvalues of the symmetric 3 x 3 S (row-major), ascending: cyclic Jacobi on the host
void sym3_eigenvalues(const double* S, double* w) {
  double a[3][3];
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) a[r][c] = S[3 * r + c];
  for (int sweep = 0; sweep < 32; ++sweep) {
    const double off = std::fabs(a[0][1]) + std::fabs(a[0][2]) + std::fabs(a[1][2]);
    if (off <= 1e-300 || off <= 1e-18 * (std::fabs(a[0][0]) + std::fabs(a[1][1]) + std::fabs(a[2][2]))) break;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        if (a[p][q] == 0.0) continue;
        const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 3; ++k) {   // columns p, q
          const double akp = a[k][p], akq = a[k][q];
          a[k][p] = c * akp - s * akq; a[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 3; ++k) {   // rows p, q
          const double apk = a[p][k], aqk = a[q][k];
          a[p][k] = c * apk - s * aqk; a[q][k] = s * apk + c * aqk;
        }
      }
  }
  w[0] = a[0][0]; w[1] = a[1][1]; w[2] = a[2][2];
  std::sort(w, w + 3);
}

}  // namespace
}  // namespace thip

using namespace thip;

extern "C" int theia_hip_linear_rotations(int32_t num_views, int32_t num_edges, const int32_t* edges,
                                          const double* relative_rotations, const theia_linear_rotation_options* options,
                                          double* orientations_out, uint8_t* estimated_out,
                                          theia_linear_rotation_summary* summary) {
  const auto t_start = std::chrono::steady_clock::now();
  const int n = num_views, E = num_edges;
  if (!summary) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null summary");
  *summary = theia_linear_rotation_summary{};
  theia_linear_rotation_options o{1000, 0, 1e-10};
  if (options) o = *options;
  // ---- refusals, before the device is touched
  if (n < 1 || !orientations_out || !estimated_out) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "no views, or a null output");
  if (E < 1 || !edges || !relative_rotations)   // CHECK_GT(constraint_entries_.size(), 0) (linear_rotation_estimator.cc:158)
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "no relative rotation constraints");
  if (o.max_num_iterations <= 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "max_num_iterations must be > 0");
  if (!(o.subspace_convergence_threshold > 0.0) || !std::isfinite(o.subspace_convergence_threshold))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "subspace_convergence_threshold must be positive and finite");
  std::vector<int> root;
  if (int bad = view_graph_components(n, E, edges, &root)) return bad;
  std::vector<uint8_t> no_edge(n, 1);   // the views outside the system: what the plan calls fixed
  for (int e = 0; e < E; ++e) {
    const int i = edges[2 * e], j = edges[2 * e + 1];
    if (i == j) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "edge %d joins view %d to itself", e, i);
    no_edge[i] = no_edge[j] = 0;
  }
  for (int v = 0; v < n; ++v)
    if (!no_edge[v] && root[v] != root[edges[0]])
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "the view graph is not connected: no path from view %d to view %d", edges[0], v);
  ViewGraphPlan g;
  fill_view_graph_lists(n, no_edge, E, edges, &g);
  const int m = g.m;
  if ((long long)m * 3 + 1 > INT32_MAX / 2) return set_error(THEIA_HIP_ERR_OUT_OF_MEMORY, "%d views: the dense system does not fit", m);
  const int n3 = 3 * m;

  int rc;
  if ((rc = thip::ensure_device())) return rc;
  theia_linear_rotation_summary sm{};
  sm.num_views_in_system = m;
  hipStream_t st = nullptr;
  DenseSpd M;   // row n3: the factorisation's right-hand-side row (zero, unused)
  DeviceViewGraph dg;
  DevBuf<double> d_rel, d_R, d_x, d_b, d_y, d_T, d_aa;
  DevBuf<LinearState> d_st;
  // the dense system first: when it does not fit, that is the answer
  if ((rc = M.alloc(n3, 1)) || (rc = d_rel.up(relative_rotations, 3 * (size_t)E)) || (rc = d_R.alloc(9 * (size_t)E)) ||
      (rc = dg.up(g, edges, E, n)) || (rc = d_x.alloc(3 * (size_t)n3)) || (rc = d_b.alloc(3 * (size_t)n3)) ||
      (rc = d_y.alloc(3 * (size_t)n3)) || (rc = d_T.alloc(3 * (size_t)n3)) || (rc = d_aa.alloc(3 * (size_t)m)) ||
      (rc = d_st.alloc(1)))
    return rc;

  // ---- set-up: R_e, M, the shift, the start block
  if ((rc = M.clear(st, true))) return rc;
  HIP_TRY(hipMemsetAsync(d_st.p, 0, sizeof(LinearState), st));
  k_rel_matrices<<<grid_of(E, kThreads), kThreads, 0, st>>>(E, d_rel.p, d_R.p);
  k_lin_assemble<<<grid_of((size_t)m + g.P, kThreads), kThreads, 0, st>>>(dg.lists, M.lda, d_R.p, M.A());
  k_shift<kThreads><<<1, kThreads, 0, st>>>(n3, M.lda, M.A(), 1.0, nullptr, nullptr, &d_st.p->shift, &d_st.p->max_diag);
  k_start_block<<<1, kThreads, 0, st>>>(n3, d_x.p, d_b.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  sm.setup_ms = ms_since(t_start);

  // ---- factor M + mu I once
  const auto t_factor = std::chrono::steady_clock::now();
  M.factor(1, st);
  bool failed = false;
  LinearState hs{};
  if ((rc = M.failed(&failed))) return rc;
  HIP_TRY(hipMemcpy(&hs, d_st.p, sizeof(LinearState), hipMemcpyDeviceToHost));
  sm.factor_ms = ms_since(t_factor);
  sm.shift = hs.shift;
  if (failed) {   // nothing to project: the outputs stay as passed in
    *summary = sm;
    return set_error(THEIA_HIP_ERR_INTERNAL, "the Cholesky factorisation of M + mu I failed (mu = %g)", hs.shift);
  }

  // ---- block inverse iteration, then the projection of whatever it reached
  const auto t_iterate = std::chrono::steady_clock::now();
  const int* done = &d_st.p->done;
  rc = run_until_done(o.max_num_iterations, kChunk, d_st.p, &hs, [&]() {
    M.solve_factored(3, d_b.p, d_T.p, d_y.p, st, done);
    k_subspace_step<<<1, kThreads, 0, st>>>(n3, d_y.p, d_x.p, d_b.p, o.subspace_convergence_threshold, d_st.p);
    return 0;
  });
  if (rc) return rc;
  k_project_so3<<<grid_of(m, kThreads), kThreads, 0, st>>>(m, n3, d_x.p, d_aa.p);
  HIP_TRY(hipGetLastError());
  std::vector<double> aa(3 * (size_t)m);
  HIP_TRY(hipMemcpy(aa.data(), d_aa.p, sizeof(double) * aa.size(), hipMemcpyDeviceToHost));
  sm.iterate_ms = ms_since(t_iterate);
  sm.iterations = hs.iterations;
  sm.subspace_change = hs.change;
  {
    double S[9], theta[3];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) S[3 * r + c] = 0.5 * (hs.H[3 * r + c] + hs.H[3 * c + r]);
    sym3_eigenvalues(S, theta);
    for (int k = 0; k < 3; ++k) sm.eigenvalues[k] = 1.0 / theta[k] - hs.shift;
    std::sort(sm.eigenvalues, sm.eigenvalues + 3);
  }
  for (int v = 0; v < n; ++v) {
    estimated_out[v] = g.idx[v] >= 0;
    if (g.idx[v] < 0) continue;
    for (int c = 0; c < 3; ++c) orientations_out[3 * (size_t)v + c] = aa[3 * (size_t)g.idx[v] + c];
  }
  *summary = sm;
  if (!hs.converged)
    return set_error(THEIA_HIP_ERR_INTERNAL, "no convergence within %d iterations: the subspace still moves by %g (threshold %g)",
                     hs.iterations, hs.change, o.subspace_convergence_threshold);
  return 0;
}
