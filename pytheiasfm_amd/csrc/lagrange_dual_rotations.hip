// lagrange_dual_rotations.hip -- LagrangeDualRotationEstimator (global_pose_estimation/lagrange_dual_rotation_estimator.cc
// :51-197 with math/rank_restricted_sdp_solver.cc:58-129, math/riemannian_staircase.cc:57-319, math/bcm_sdp_solver.h:64-72
// and math/rotation.cc:105-120; Eriksson et al., "Rotation Averaging and Strong Duality"; the Riemannian staircase of
// SE-Sync): global orientations from the pairs' relative rotations alone, without an initial guess, with a certificate
// of global optimality, on the device in FP64.
//
// Per pair e = (i, j) with R_e = AngleAxisToRotationMatrix(rotation_2), R_j ~ R_e R_i, the symmetric 3n x 3n matrix R has
// R_e' at block (i, j) and R_e at block (j, i); Q = -R.  The unknown is Y [r][3n], one r x 3 block with orthonormal
// columns per view; the method minimises f = tr(Y Q Y') by block coordinate minimisation (BCM), tests lambda_min of
// S = Q - SymBlockDiag(Q Y' Y) and, while that is negative, adds a row to Y and leaves the saddle along an eigenvector.
//
// Stages:
//   plan (host)        the views with edges indexed compactly in view order; per view its neighbours in ascending order
//                      with the 3 x 3 block Q_ji per directed entry; the sweep order (INDEX or COLOURED) and its levels:
//                      level(i) = 1 + max level of the neighbours earlier in the order, so that no two views of a level
//                      share an edge and every earlier neighbour lies in a lower level
//   k_sweep_levels     the hot path.  One wavefront per view of a level: the lanes stride over the neighbour list and
//                      accumulate Y_j Q_ji, a butterfly sums the 3 r entries over the wave, and every lane takes the polar
//                      factor of -G_i (one-sided Jacobi over the three columns, one Newton-Schulz step); [I_3; 0] for a
//                      zero block.  A level of more than kSmallLevel views is one launch; a run of smaller levels is
//                      walked by one workgroup with a workgroup barrier between levels (a bounded loop: no flag, no spin)
//   k_gather           one wavefront per view: G_i from the final Y, <Y_i, G_i> and the squared norm of the Riemannian
//                      gradient 2 (G_i - Y_i sym(Y_i' G_i))
//   k_bcm_state        one workgroup: f = sum_i <Y_i, G_i> in a fixed tree, the reference's stopping test
//                      |f_prev - f| / max(|f_prev|, 1) <= tolerance, the sweep count and the `done` flag that every later
//                      launch of a chunk tests first (run_until_done, device_util.h)
//   certificate        k_cert_assemble writes the lower triangle of S + sigma I (DenseSpd); the FP64-MFMA Cholesky factors
//                      it; no failed pivot at sigma = tolerance means lambda_min > -tolerance: certified.  Otherwise sigma
//                      grows by 4 until a factorisation succeeds and is bisected (geometrically) until the failing and
//                      the succeeding shift differ by 5 %: lambda_min lies in (-sigma_ok, -sigma_fail].  Inverse iteration
//                      through the last factor (smallest_eigenvector.h's k_iterate) gives v; k_rayleigh evaluates v' S v
//                      from the sparse blocks, and v is admitted when v' S v <= -0.9 sigma_ok <= 0.9 lambda_min
//   escape             k_retract: per view the polar factor of [Y_i; alpha v_i']; the reference's backtracking over alpha
//                      on the host, one k_gather and one read of (f, |grad|^2) per trial
//   k_solution         one thread per view: Y_0' Y_i, ProjectToSOd when the rank left behind is above min_rank, the
//                      transpose, negated when its determinant is negative, RotationMatrixToAngleAxis
//
// Deviations from the reference, all stated in include/theia_hip.h: G_i is gathered at every update instead of kept
// incrementally; the certificate is a factorisation, not a Lanczos eigenvalue, and the escape direction is the inverse
// iteration's (the reference's starts from a random vector); the gauge view is the lowest view that has an edge.
//
// The polar factor is defined and tested where sigma_min(G_i) >= 1e-3 sigma_max(G_i): there |Y_i' Y_i - I| stayed below
// 4e-16 and the distance from numpy's U V' below 5e-14 (tests/test_lagrange_dual_rotations_gpu.py).  Below that nothing
// is promised:
// the columns are still normalised one by one and re-orthogonalised by the Newton-Schulz step, but how far the result
// lies from the SVD's U V' has not been examined.  A non-zero block with an exactly zero singular value divides by it, f
// becomes non-finite, and the call stops with THEIA_HIP_ERR_INTERNAL.
//
// Determinism: no atomics.  Every G_i is a sum in a fixed lane order and a fixed butterfly, f a fixed tree (block_sum),
// every entry of S has one writer.  Two runs on one input are bit-identical.
#include "small_linalg.h"
#include "rotation_maps.h"
#include "dense_cholesky.h"
#include "smallest_eigenvector.h"
#include "view_graph_plan.h"
#include "wave_reduce.h"

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <type_traits>
#include <utility>
#include <vector>

namespace thip {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = 8;          // sweeps enqueued between two reads of the `done` flag
constexpr int kSmallLevel = 16;    // a level of at most this many views joins a run walked by one workgroup
constexpr int kMaxRank = 11;       // max_rank <= 10, and the row the reference adds after an uncertified last level
constexpr int kStride = 3 * kMaxRank;   // doubles per view in Y and G: block i at 33 i, entry (row k, column c) at 3 k + c

struct BcmState {
  int done, sweeps, nonfinite, pad;
  double f, f_prev, err, tolerance;
};

// The adjacency as the kernels read it.  view / owner: compact indices; q[9 k ..]: Q_ji row-major for the
// entry k of owner i with neighbour j, so that G_i = sum_k Y_j Q_ji.
struct Adjacency {
  int m, entries;
  const int* off;
  const int* view;
  const int* owner;
  const double* q;
};

// U V' of the thin SVD of the non-zero R x 3 block A (row-major, in place).  One-sided Jacobi: the columns are rotated
// until they are orthogonal (A V = U Sigma), then U V' = sum_k (A V)_k / sigma_k V_k'.  One Newton-Schulz step
// Y (3 I - Y' Y) / 2 squares what is left of |Y' Y - I|.
template <int R>
__device__ __forceinline__ void polar_factor(double* A) {
  double V[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int pq = 0; pq < 3; ++pq) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
      double a = 0.0, b = 0.0, g = 0.0;
#pragma unroll
      for (int k = 0; k < R; ++k) { a += A[3 * k + p] * A[3 * k + p]; b += A[3 * k + q] * A[3 * k + q]; g += A[3 * k + p] * A[3 * k + q]; }
      if (fabs(g) > DBL_EPSILON * sqrt(a * b)) {
        rotated = true;
        const double zeta = (b - a) / (2.0 * g);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
        for (int k = 0; k < R; ++k) {
          const double x = A[3 * k + p], y = A[3 * k + q];
          A[3 * k + p] = c * x - s * y; A[3 * k + q] = s * x + c * y;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double x = V[3 * k + p], y = V[3 * k + q];
          V[3 * k + p] = c * x - s * y; V[3 * k + q] = s * x + c * y;
        }
      }
    }
    if (!rotated) break;
  }
  double inv[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double a = 0.0;
#pragma unroll
    for (int k = 0; k < R; ++k) a += A[3 * k + c] * A[3 * k + c];
    inv[c] = 1.0 / sqrt(a);
  }
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const double u0 = A[3 * k] * inv[0], u1 = A[3 * k + 1] * inv[1], u2 = A[3 * k + 2] * inv[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) A[3 * k + c] = (u0 * V[3 * c] + u1 * V[3 * c + 1]) + u2 * V[3 * c + 2];
  }
  double M[9];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < R; ++k) s += A[3 * k + a] * A[3 * k + b];
      M[3 * a + b] = (a == b ? 1.5 : 0.0) - 0.5 * s;
    }
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const double y0 = A[3 * k], y1 = A[3 * k + 1], y2 = A[3 * k + 2];
#pragma unroll
    for (int c = 0; c < 3; ++c) A[3 * k + c] = (y0 * M[c] + y1 * M[3 + c]) + y2 * M[6 + c];
  }
}

// G_i = sum over the neighbours of Y_j Q_ji, in every lane of the wave: lane l takes the entries l, l + 64, ... of the
// list in order, the butterfly adds the lanes.  Y is read through a plain pointer: a run of levels reads what earlier
// levels of the same launch wrote.
template <int R>
__device__ __forceinline__ void gather_block(const Adjacency& adj, int i, const double* Y, double* acc) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int t = 0; t < 3 * R; ++t) acc[t] = 0.0;
  for (int k = adj.off[i] + lane; k < adj.off[i + 1]; k += 64) {
    const double* y = Y + (size_t)kStride * adj.view[k];
    double q[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) q[t] = adj.q[9 * (size_t)k + t];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const double y0 = y[3 * r], y1 = y[3 * r + 1], y2 = y[3 * r + 2];
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[3 * r + c] += (y0 * q[c] + y1 * q[3 + c]) + y2 * q[6 + c];
    }
  }
#pragma unroll
  for (int t = 0; t < 3 * R; ++t) acc[t] = wave_sum_butterfly(acc[t]);
}

// The levels [l0, l1) of one sweep.  gridDim.x > 1 only for a single level.  order[level_off[l] .. level_off[l + 1]):
// the views of level l.
template <int R>
__global__ __launch_bounds__(kThreads) void k_sweep_levels(Adjacency adj, const int* __restrict__ level_off,
                                                           const int* __restrict__ order, int l0, int l1, double* Y,
                                                           const BcmState* __restrict__ st) {
  if (st->done) return;   // workgroup-uniform, before any barrier
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int l = l0; l < l1; ++l) {
    const int end = level_off[l + 1];
    for (int p = level_off[l] + blockIdx.x * kWaves + wave; p < end; p += gridDim.x * kWaves) {
      const int i = order[p];
      double A[3 * R];
      gather_block<R>(adj, i, Y, A);
      bool zero = true;
#pragma unroll
      for (int t = 0; t < 3 * R; ++t) { zero = zero && A[t] == 0.0; A[t] = -A[t]; }
      if (zero) {
#pragma unroll
        for (int t = 0; t < 3 * R; ++t) A[t] = (t < 9 && t % 4 == 0) ? 1.0 : 0.0;
      } else {
        polar_factor<R>(A);
      }
      if (lane == 0) {
#pragma unroll
        for (int t = 0; t < 3 * R; ++t) Y[(size_t)kStride * i + t] = A[t];
      }
    }
    if (l + 1 < l1) __syncthreads();
  }
}

// One wavefront per view: G_i, <Y_i, G_i> and |2 (G_i - Y_i sym(Y_i' G_i))|_F^2.  st (optional): skipped while done.
template <int R>
__global__ __launch_bounds__(kThreads) void k_gather(Adjacency adj, const double* __restrict__ Y, double* __restrict__ G,
                                                     double* __restrict__ fpart, double* __restrict__ gpart,
                                                     const BcmState* __restrict__ st) {
  if (st && st->done) return;
  const int i = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (i >= adj.m) return;
  double A[3 * R];
  gather_block<R>(adj, i, Y, A);
  if ((threadIdx.x & 63) != 0) return;
  const double* y = Y + (size_t)kStride * i;
  double f = 0.0, P[9];
#pragma unroll
  for (int t = 0; t < 3 * R; ++t) { G[(size_t)kStride * i + t] = A[t]; f += y[t] * A[t]; }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < R; ++k) s += y[3 * k + a] * A[3 * k + b];
      P[3 * a + b] = s;
    }
  double g2 = 0.0;
#pragma unroll
  for (int k = 0; k < R; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double ys = (y[3 * k] * (0.5 * (P[c] + P[3 * c])) + y[3 * k + 1] * (0.5 * (P[3 + c] + P[3 * c + 1]))) +
                        y[3 * k + 2] * (0.5 * (P[6 + c] + P[3 * c + 2]));
      const double d = 2.0 * (A[3 * k + c] - ys);
      g2 += d * d;
    }
  fpart[i] = f;
  gpart[i] = g2;
}

// One workgroup.  start: the state of a new BCM (f_prev = DBL_MAX, no sweep yet); otherwise the sweep just gathered.
__global__ __launch_bounds__(kThreads) void k_bcm_state(int m, const double* __restrict__ fpart, int start, BcmState* st) {
  __shared__ double red[kThreads];
  if (!start && st->done) return;
  double s = 0.0;
  for (int k = threadIdx.x; k < m; k += kThreads) s += fpart[k];
  const double f = block_sum<kThreads>(s, red);
  if (threadIdx.x != 0) return;
  const double f_prev = start ? DBL_MAX : st->f;
  const double err = fabs(f_prev - f) / fmax(fabs(f_prev), 1.0);
  st->f_prev = f_prev;
  st->f = f;
  st->err = err;
  st->sweeps = start ? 0 : st->sweeps + 1;
  st->nonfinite = !isfinite(f);
  st->done = (err <= st->tolerance || !isfinite(f)) ? 1 : 0;
}

// One workgroup: out[0] = sum a, out[1] = sum b (b optional), fixed trees.
__global__ __launch_bounds__(kThreads) void k_sum2(int m, const double* __restrict__ a, const double* __restrict__ b,
                                                   double* __restrict__ out) {
  __shared__ double red[kThreads];
  double sa = 0.0, sb = 0.0;
  for (int k = threadIdx.x; k < m; k += kThreads) { sa += a[k]; if (b) sb += b[k]; }
  const double ra = block_sum<kThreads>(sa, red), rb = block_sum<kThreads>(sb, red);
  if (threadIdx.x == 0) { out[0] = ra; out[1] = rb; }
}

// Lambda_i = sym(G_i' Y_i), row-major
__device__ __forceinline__ void lambda_block(int rank, const double* __restrict__ y, const double* __restrict__ g, double* L) {
  double P[9];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      double s = 0.0;
      for (int k = 0; k < rank; ++k) s += g[3 * k + a] * y[3 * k + b];
      P[3 * a + b] = s;
    }
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) L[3 * a + b] = 0.5 * (P[3 * a + b] + P[3 * b + a]);
}

// The lower triangle of S + sigma I into the zeroed array.  Thread t < m: the diagonal block -Lambda_t + sigma I.
// Thread m + k: the adjacency entry k of owner i with neighbour j < i: block (i, j) = Q_ij = Q_ji'.
__global__ __launch_bounds__(kThreads) void k_cert_assemble(Adjacency adj, int rank, const double* __restrict__ Y,
                                                            const double* __restrict__ G, double sigma, int lda,
                                                            double* __restrict__ M) {
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t < adj.m) {
    double L[9];
    lambda_block(rank, Y + (size_t)kStride * t, G + (size_t)kStride * t, L);
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b <= a; ++b) M[(size_t)(3 * t + a) * lda + 3 * t + b] = (a == b ? sigma : 0.0) - L[3 * a + b];
  } else if (t < adj.m + adj.entries) {
    const int k = t - adj.m, i = adj.owner[k], j = adj.view[k];
    if (i > j) {
      const double* q = adj.q + 9 * (size_t)k;
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) M[(size_t)(3 * i + r) * lda + 3 * j + c] = q[3 * c + r];
    }
  }
}

// One workgroup: the start vector of the inverse iteration (the hashed entries of linear_rotations.hip's start block,
// normalised) into x and b, and the state with its shift.
__global__ __launch_bounds__(kThreads) void k_cert_start(int n, double shift, double* __restrict__ x, double* __restrict__ b,
                                                         InverseIterationState* __restrict__ st) {
  __shared__ double red[kThreads];
  double s = 0.0;
  for (int r = threadIdx.x; r < n; r += kThreads) {
    const unsigned h = (3u * (unsigned)r + 1u) * 2654435761u;
    const double v = (double)(h >> 8) * 0x1p-23 - 1.0;
    x[r] = v;
    s += v * v;
  }
  const double norm = sqrt(block_sum<kThreads>(s, red));
  for (int r = threadIdx.x; r < n; r += kThreads) { x[r] /= norm; b[r] = x[r]; }
  if (threadIdx.x == 0) {
    *st = InverseIterationState{};
    st->shift = shift;
  }
}

// One thread per view: part[i] = v_i . (S v)_i with (S v)_i = sum_k Q_ij v_j - Lambda_i v_i.
__global__ __launch_bounds__(kThreads) void k_rayleigh(Adjacency adj, int rank, const double* __restrict__ Y,
                                                       const double* __restrict__ G, const double* __restrict__ v,
                                                       double* __restrict__ part) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= adj.m) return;
  double L[9], w[3];
  lambda_block(rank, Y + (size_t)kStride * i, G + (size_t)kStride * i, L);
  const double* vi = v + 3 * (size_t)i;
  for (int r = 0; r < 3; ++r) w[r] = -((L[3 * r] * vi[0] + L[3 * r + 1] * vi[1]) + L[3 * r + 2] * vi[2]);
  for (int k = adj.off[i]; k < adj.off[i + 1]; ++k) {
    const double* q = adj.q + 9 * (size_t)k;
    const double* vj = v + 3 * (size_t)adj.view[k];
    for (int r = 0; r < 3; ++r) w[r] += (q[r] * vj[0] + q[3 + r] * vj[1]) + q[6 + r] * vj[2];
  }
  part[i] = (vi[0] * w[0] + vi[1] * w[1]) + vi[2] * w[2];
}

// One thread per view: Yt_i = the polar factor of [Y_i; alpha v_i'] at R rows (Y_i has R - 1); alpha == 0: the block
// with its zero row, unchanged.
template <int R>
__global__ __launch_bounds__(kThreads) void k_retract(int m, double alpha, const double* __restrict__ v,
                                                      const double* __restrict__ Y, double* __restrict__ Yt) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= m) return;
  double A[3 * R];
#pragma unroll
  for (int t = 0; t < 3 * (R - 1); ++t) A[t] = Y[(size_t)kStride * i + t];
#pragma unroll
  for (int c = 0; c < 3; ++c) A[3 * (R - 1) + c] = alpha * v[3 * (size_t)i + c];
  if (alpha != 0.0) polar_factor<R>(A);
#pragma unroll
  for (int t = 0; t < 3 * R; ++t) Yt[(size_t)kStride * i + t] = A[t];
}

// One thread per view: X_i = Y_0' Y_i, ProjectToSOd (math/rotation.cc:105-120) when `rounded`, the orientation.
template <int R>
__global__ __launch_bounds__(kThreads) void k_solution(int m, int rounded, const double* __restrict__ Y, double* __restrict__ aa) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= m) return;
  const double* y0 = Y;
  const double* y = Y + (size_t)kStride * i;
  double B[9], Rm[9];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < R; ++k) s += y0[3 * k + a] * y[3 * k + b];
      B[3 * a + b] = s;
    }
  if (rounded) {
    double U[9], S[3], V[9];
    rsc::svd_sq<3>(B, U, S, V);
    if (rsc::det3(U) * rsc::det3(V) <= 0.0) { U[2] = -U[2]; U[5] = -U[5]; U[8] = -U[8]; }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) B[3 * r + c] = (U[3 * r] * V[3 * c] + U[3 * r + 1] * V[3 * c + 1]) + U[3 * r + 2] * V[3 * c + 2];
  }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) Rm[3 * r + c] = B[3 * c + r];
  if (rsc::det3(Rm) < 0.0) {
#pragma unroll
    for (int q = 0; q < 9; ++q) Rm[q] = -Rm[q];
  }
  double o[3];
  rsc::rot_to_angle_axis(Rm, o);
  aa[3 * (size_t)i] = o[0]; aa[3 * (size_t)i + 1] = o[1]; aa[3 * (size_t)i + 2] = o[2];
}

// calls body(std::integral_constant<int, R>) for the run-time rank in [LO, HI]
template <int LO, int HI, class Body>
inline void with_rank(int rank, Body&& body) {
  if constexpr (LO <= HI) {
    if (rank == LO) body(std::integral_constant<int, LO>{});
    else with_rank<LO + 1, HI>(rank, body);
  }
}

// One run of consecutive levels: one launch.
struct SweepLaunch { int l0, l1, grid; };

// The sweep order, its levels and its launches.  order: INDEX = 0 .. m-1; COLOURED = by (greedy colour in index order,
// index).  The views come out sorted by (level, position in the order).
struct SweepPlan {
  std::vector<int> order, level_off;
  std::vector<SweepLaunch> launches;
  int levels = 0;

  void build(int m, const std::vector<int>& off, const std::vector<int>& view, bool coloured) {
    std::vector<int> seq(m), pos(m), level(m, 0);
    for (int i = 0; i < m; ++i) seq[i] = i;
    if (coloured) {
      std::vector<int> colour(m, -1), mark(m + 1, -1);
      for (int i = 0; i < m; ++i) {
        for (int k = off[i]; k < off[i + 1]; ++k) if (colour[view[k]] >= 0) mark[colour[view[k]]] = i;
        int c = 0;
        while (mark[c] == i) ++c;
        colour[i] = c;
      }
      std::stable_sort(seq.begin(), seq.end(), [&](int a, int b) { return colour[a] < colour[b]; });
    }
    for (int p = 0; p < m; ++p) pos[seq[p]] = p;
    levels = 0;
    for (int p = 0; p < m; ++p) {
      const int i = seq[p];
      int l = 0;
      for (int k = off[i]; k < off[i + 1]; ++k) if (pos[view[k]] < p) l = std::max(l, level[view[k]] + 1);
      level[i] = l;
      levels = std::max(levels, l + 1);
    }
    level_off.assign(levels + 1, 0);
    for (int i = 0; i < m; ++i) ++level_off[level[i] + 1];
    for (int l = 0; l < levels; ++l) level_off[l + 1] += level_off[l];
    order.resize(m);
    std::vector<int> fill(level_off.begin(), level_off.end() - 1);
    for (int p = 0; p < m; ++p) order[fill[level[seq[p]]]++] = seq[p];
    launches.clear();
    for (int l = 0; l < levels;) {
      const int size = level_off[l + 1] - level_off[l];
      if (size > kSmallLevel) { launches.push_back({l, l + 1, (size + kWaves - 1) / kWaves}); ++l; continue; }
      int l1 = l + 1;
      while (l1 < levels && level_off[l1 + 1] - level_off[l1] <= kSmallLevel) ++l1;
      launches.push_back({l, l1, 1});
      l = l1;
    }
  }
};

}  // namespace
}  // namespace thip

using namespace thip;

extern "C" int theia_hip_lagrange_dual_rotations(int32_t num_views, int32_t num_edges, const int32_t* edges,
                                                 const double* relative_rotations,
                                                 const theia_lagrange_dual_options* options, int32_t rank_init,
                                                 const double* y_init, double* orientations_out, uint8_t* estimated_out,
                                                 double* y_out, theia_lagrange_dual_summary* summary,
                                                 double* level_log_out, int32_t level_log_rows) {
  const auto t_start = std::chrono::steady_clock::now();
  const int n = num_views, E = num_edges;
  if (!summary) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null summary");
  *summary = theia_lagrange_dual_summary{};
  theia_lagrange_dual_options o{THEIA_SDP_RIEMANNIAN_STAIRCASE, 500, 3, 10, THEIA_SWEEP_ORDER_INDEX, 0, 1e-8, 1e-5, 1e-2, 1e-4};
  if (options) o = *options;
  // ---- refusals, before the device is touched
  if (n < 1 || !orientations_out || !estimated_out) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "no views, or a null output");
  if (E < 1 || !edges || !relative_rotations)   // CHECK_GT(view_pairs.size(), 0) (lagrange_dual_rotation_estimator.cc:91)
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "no relative rotation constraints");
  if (o.solver_type == THEIA_SDP_RBR_BCM)
    return set_error(THEIA_HIP_ERR_UNSUPPORTED, "RBR_BCM is not built: its dense 3n x 3n iterate is another design");
  if (o.solver_type != THEIA_SDP_RANK_DEFICIENT_BCM && o.solver_type != THEIA_SDP_RIEMANNIAN_STAIRCASE)
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "unknown solver_type %d", o.solver_type);
  if (o.sweep_order != THEIA_SWEEP_ORDER_INDEX && o.sweep_order != THEIA_SWEEP_ORDER_COLOURED)
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "unknown sweep_order %d", o.sweep_order);
  if (o.max_iterations <= 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "max_iterations must be > 0");
  if (o.min_rank < 3 || o.max_rank > 10 || o.min_rank > o.max_rank)
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "min_rank .. max_rank = %d .. %d is not inside 3 .. 10", o.min_rank, o.max_rank);
  for (double t : {o.tolerance, o.min_eigenvalue_nonnegativity_tolerance, o.gradient_tolerance, o.preconditioned_gradient_tolerance})
    if (!(t >= 0.0) || !std::isfinite(t)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "a tolerance is negative or not finite");
  if (y_init && (rank_init < 3 || rank_init > 10))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "rank_init = %d is not inside 3 .. 10", rank_init);
  const bool staircase = o.solver_type == THEIA_SDP_RIEMANNIAN_STAIRCASE;
  if (y_init && staircase && (rank_init < o.min_rank || rank_init > o.max_rank))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "rank_init = %d is outside min_rank .. max_rank = %d .. %d", rank_init, o.min_rank, o.max_rank);
  std::vector<int> root;
  if (int bad = view_graph_components(n, E, edges, &root)) return bad;
  if (int bad = check_pairs(n, E, edges)) return bad;   // a self pair; a pair given twice in either direction
  std::vector<uint8_t> no_edge(n, 1);
  for (int e = 0; e < E; ++e) no_edge[edges[2 * e]] = no_edge[edges[2 * e + 1]] = 0;
  for (int v = 0; v < n; ++v)
    if (!no_edge[v] && root[v] != root[edges[0]])
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "the view graph is not connected: no path from view %d to view %d", edges[0], v);

  // ---- plan: compact indices, the adjacency in ascending neighbour order, the sweep's levels
  std::vector<int> idx(n, -1), live;
  for (int v = 0; v < n; ++v) if (!no_edge[v]) { idx[v] = (int)live.size(); live.push_back(v); }
  const int m = (int)live.size(), n3 = 3 * m;
  if ((long long)m * 3 + 1 > INT32_MAX / 2) return set_error(THEIA_HIP_ERR_OUT_OF_MEMORY, "%d views: the dense certificate does not fit", m);
  std::vector<int> off(m + 1, 0), adj_view(2 * (size_t)E), adj_owner(2 * (size_t)E), adj_edge(2 * (size_t)E);
  {
    std::vector<std::pair<int64_t, int>> ent;   // (owner * m + neighbour, 2 e + side)
    ent.reserve(2 * (size_t)E);
    for (int e = 0; e < E; ++e) {
      const int a = idx[edges[2 * e]], b = idx[edges[2 * e + 1]];
      ent.emplace_back((int64_t)a * m + b, 2 * e);       // owner = the pair's first view: Q_ji = -R_e
      ent.emplace_back((int64_t)b * m + a, 2 * e + 1);   // owner = its second view: Q_ji = -R_e'
    }
    std::sort(ent.begin(), ent.end());
    for (size_t k = 0; k < ent.size(); ++k) {
      adj_owner[k] = (int)(ent[k].first / m); adj_view[k] = (int)(ent[k].first % m); adj_edge[k] = ent[k].second;
      ++off[adj_owner[k] + 1];
    }
    for (int i = 0; i < m; ++i) off[i + 1] += off[i];
  }
  std::vector<double> adj_q(18 * (size_t)E);
  for (size_t k = 0; k < adj_edge.size(); ++k) {
    // AngleAxisToRotationMatrix on the host: the same formula as rsc::angle_axis_to_rot
    const double* aa = relative_rotations + 3 * (size_t)(adj_edge[k] >> 1);
    double Rm[9];
    const double theta2 = aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2];
    if (theta2 > DBL_EPSILON) {
      const double theta = std::sqrt(theta2), wx = aa[0] / theta, wy = aa[1] / theta, wz = aa[2] / theta;
      const double c = std::cos(theta), s = std::sin(theta);
      Rm[0] = c + wx * wx * (1.0 - c);      Rm[3] = wz * s + wx * wy * (1.0 - c);  Rm[6] = -wy * s + wx * wz * (1.0 - c);
      Rm[1] = wx * wy * (1.0 - c) - wz * s; Rm[4] = c + wy * wy * (1.0 - c);       Rm[7] = wx * s + wy * wz * (1.0 - c);
      Rm[2] = wy * s + wx * wz * (1.0 - c); Rm[5] = -wx * s + wy * wz * (1.0 - c); Rm[8] = c + wz * wz * (1.0 - c);
    } else {
      Rm[0] = 1.0; Rm[3] = aa[2]; Rm[6] = -aa[1];
      Rm[1] = -aa[2]; Rm[4] = 1.0; Rm[7] = aa[0];
      Rm[2] = aa[1]; Rm[5] = -aa[0]; Rm[8] = 1.0;
    }
    double* q = adj_q.data() + 9 * k;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) q[3 * r + c] = (adj_edge[k] & 1) ? -Rm[3 * c + r] : -Rm[3 * r + c];
  }
  SweepPlan plan;
  plan.build(m, off, adj_view, o.sweep_order == THEIA_SWEEP_ORDER_COLOURED);

  int rc;
  if ((rc = thip::ensure_device())) return rc;
  theia_lagrange_dual_summary sm{};
  sm.num_views_in_system = m;
  sm.gauge_view = live[0];
  sm.schedule_levels = plan.levels;
  sm.schedule_launches = (int)plan.launches.size();
  hipStream_t st = nullptr;
  DenseSpd M;
  DevBuf<int> d_off, d_view, d_owner, d_order, d_level_off;
  DevBuf<double> d_q, d_Y, d_Yt, d_G, d_fpart, d_gpart, d_sums, d_x, d_b, d_y, d_T, d_aa;
  DevBuf<BcmState> d_st;
  DevBuf<InverseIterationState> d_it;
  // the dense certificate first: when it does not fit, that is the answer
  if (staircase && (rc = M.alloc(n3, 1))) return rc;
  if ((rc = d_off.up(off.data(), off.size())) || (rc = d_view.up(adj_view.data(), adj_view.size())) ||
      (rc = d_owner.up(adj_owner.data(), adj_owner.size())) || (rc = d_q.up(adj_q.data(), adj_q.size())) ||
      (rc = d_order.up(plan.order.data(), plan.order.size())) || (rc = d_level_off.up(plan.level_off.data(), plan.level_off.size())) ||
      (rc = d_Y.alloc((size_t)kStride * m)) || (rc = d_Yt.alloc((size_t)kStride * m)) || (rc = d_G.alloc((size_t)kStride * m)) ||
      (rc = d_fpart.alloc(m)) || (rc = d_gpart.alloc(m)) || (rc = d_sums.alloc(2)) || (rc = d_aa.alloc(3 * (size_t)m)) ||
      (rc = d_st.alloc(1)) || (rc = d_it.alloc(1)))
    return rc;
  if (staircase && ((rc = d_x.alloc(n3)) || (rc = d_b.alloc(n3)) || (rc = d_y.alloc(n3)) || (rc = d_T.alloc(n3)))) return rc;
  const Adjacency adj{m, 2 * E, d_off.p, d_view.p, d_owner.p, d_q.p};

  int rank = y_init ? rank_init : (staircase ? o.min_rank : 3);
  {
    std::vector<double> Y0((size_t)kStride * m, 0.0);
    if (y_init)
      for (int i = 0; i < m; ++i)
        for (int k = 0; k < rank; ++k)
          for (int c = 0; c < 3; ++c) Y0[(size_t)kStride * i + 3 * k + c] = y_init[(size_t)k * n3 + 3 * i + c];
    HIP_TRY(hipMemcpy(d_Y.p, Y0.data(), sizeof(double) * Y0.size(), hipMemcpyHostToDevice));
  }
  sm.setup_ms = ms_since(t_start);

  const int wave_grid = grid_of(m, kWaves), view_grid = grid_of(m, kThreads);
  BcmState hs{};
  auto gather = [&](int r, const double* Y, const BcmState* skip) {
    with_rank<3, kMaxRank>(r, [&](auto R) {
      k_gather<decltype(R)::value><<<wave_grid, kThreads, 0, st>>>(adj, Y, d_G.p, d_fpart.p, d_gpart.p, skip);
    });
  };
  // one BCM at `rank` from d_Y; leaves d_G = the gather of the final Y and hs = the state
  auto run_bcm = [&]() -> int {
    const auto t0 = std::chrono::steady_clock::now();
    hs = BcmState{};
    hs.tolerance = o.tolerance;
    HIP_TRY(hipMemcpyAsync(d_st.p, &hs, sizeof(BcmState), hipMemcpyHostToDevice, st));
    gather(rank, d_Y.p, nullptr);
    k_bcm_state<<<1, kThreads, 0, st>>>(m, d_fpart.p, 1, d_st.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(&hs, d_st.p, sizeof(BcmState), hipMemcpyDeviceToHost));
    int rc2 = run_until_done(o.max_iterations, kChunk, d_st.p, &hs, [&]() {
      with_rank<3, 10>(rank, [&](auto R) {
        for (const SweepLaunch& l : plan.launches)
          k_sweep_levels<decltype(R)::value><<<l.grid, kThreads, 0, st>>>(adj, d_level_off.p, d_order.p, l.l0, l.l1, d_Y.p, d_st.p);
      });
      gather(rank, d_Y.p, d_st.p);
      k_bcm_state<<<1, kThreads, 0, st>>>(m, d_fpart.p, 0, d_st.p);
      return 0;
    });
    sm.sweep_ms += ms_since(t0);
    sm.total_sweeps += hs.sweeps;
    if (rc2) return rc2;
    if (hs.nonfinite) return set_error(THEIA_HIP_ERR_INTERNAL, "f is not finite after %d sweeps at rank %d: a singular block G_i", hs.sweeps, rank);
    return 0;
  };
  // factors S + sigma I of the current (d_Y, d_G); *ok: no failed pivot
  auto try_shift = [&](double sigma, bool* ok) -> int {
    int rc2;
    if ((rc2 = M.clear(st, true))) return rc2;
    k_cert_assemble<<<grid_of((size_t)m + 2 * (size_t)E, kThreads), kThreads, 0, st>>>(adj, rank, d_Y.p, d_G.p, sigma, M.lda, M.A());
    M.factor(1, st);
    bool failed = false;
    if ((rc2 = M.failed(&failed))) return rc2;
    sm.factorisations += 1;
    *ok = !failed;
    return 0;
  };
  int num_levels = 0;
  auto log_level = [&](double sweeps, double f, double certified, double lambda_min, double rayleigh, double alpha, double fallback) {
    if (level_log_out && num_levels < level_log_rows) {
      double* row = level_log_out + 8 * (size_t)num_levels;
      row[0] = rank; row[1] = sweeps; row[2] = f; row[3] = certified; row[4] = lambda_min; row[5] = rayleigh; row[6] = alpha; row[7] = fallback;
    }
    ++num_levels;
  };

  int end_state = THEIA_LAGRANGE_DUAL_END_BCM;
  if (!staircase) {
    if ((rc = run_bcm())) return rc;
    log_level(hs.sweeps, hs.f, 0.0, NAN, NAN, 0.0, 0.0);
  } else {
    end_state = THEIA_LAGRANGE_DUAL_END_MAX_RANK;
    while (rank <= o.max_rank) {
      if ((rc = run_bcm())) return rc;
      const auto t_cert = std::chrono::steady_clock::now();
      const double tau = o.min_eigenvalue_nonnegativity_tolerance, FY = hs.f;
      bool ok = false;
      if ((rc = try_shift(tau, &ok))) return rc;
      if (ok) {
        sm.certificate_ms += ms_since(t_cert);
        sm.lambda_min = NAN;
        log_level(hs.sweeps, FY, 1.0, NAN, NAN, 0.0, 0.0);
        end_state = THEIA_LAGRANGE_DUAL_END_CERTIFIED;
        break;
      }
      // lambda_min in (-hi, -lo]: grow, then bisect to 5 %
      double lo = std::max(tau, DBL_MIN), hi = lo;
      for (int k = 0; !ok; ++k) {
        if (k == 600) return set_error(THEIA_HIP_ERR_INTERNAL, "no shift makes S + sigma I positive definite");
        hi *= 4.0;
        if ((rc = try_shift(hi, &ok))) return rc;
        if (!ok) lo = hi;
      }
      double factored = hi;
      while (hi > 1.05 * lo) {
        const double mid = std::sqrt(lo * hi);
        if ((rc = try_shift(mid, &ok))) return rc;
        factored = mid;
        if (ok) hi = mid; else lo = mid;
      }
      if (factored != hi && (rc = try_shift(hi, &ok))) return rc;
      k_cert_start<<<1, kThreads, 0, st>>>(n3, hi, d_x.p, d_b.p, d_it.p);
      InverseIterationState is{};
      const int* done = &d_it.p->done;
      rc = run_until_done(200, 8, d_it.p, &is, [&]() {
        M.solve_factored(1, d_b.p, d_T.p, d_y.p, st, done);
        k_iterate<kThreads><<<1, kThreads, 0, st>>>(n3, d_y.p, d_x.p, d_b.p, 1e-9, d_it.p);
        return 0;
      });
      if (rc) return rc;
      k_rayleigh<<<view_grid, kThreads, 0, st>>>(adj, rank, d_Y.p, d_G.p, d_x.p, d_fpart.p);
      k_sum2<<<1, kThreads, 0, st>>>(m, d_fpart.p, nullptr, d_sums.p);
      HIP_TRY(hipGetLastError());
      double sums[2];
      HIP_TRY(hipMemcpy(sums, d_sums.p, sizeof(sums), hipMemcpyDeviceToHost));
      const double rayleigh = sums[0], lambda_min = is.eigenvalue;
      sm.lambda_min = lambda_min;
      sm.certificate_ms += ms_since(t_cert);
      if (!(rayleigh <= -0.9 * hi))
        return set_error(THEIA_HIP_ERR_INTERNAL, "the inverse iteration found no direction of negative curvature: v' S v = %g, lambda_min in (%g, %g]",
                         rayleigh, -hi, -lo);
      // ---- escape (riemannian_staircase.cc:215-309): a zero row under Y, backtracking along Ydot = e_{r+1} v'
      const auto t_esc = std::chrono::steady_clock::now();
      const int r1 = rank + 1;
      auto retract = [&](double alpha) {
        with_rank<4, kMaxRank>(r1, [&](auto R) { k_retract<decltype(R)::value><<<view_grid, kThreads, 0, st>>>(m, alpha, d_x.p, d_Y.p, d_Yt.p); });
      };
      auto accept = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(d_Y.p, d_Yt.p, sizeof(double) * (size_t)kStride * m, hipMemcpyDeviceToDevice, st));
        return 0;
      };
      const double alpha_min = 1e-6;
      double alpha = std::max(16.0 * alpha_min, 10.0 * o.gradient_tolerance / std::fabs(lambda_min));
      double best_f = INFINITY, best_alpha = 0.0, accepted = 0.0;
      bool escaped = false, fallback = false;
      for (; alpha >= alpha_min; alpha /= 2.0) {
        retract(alpha);
        gather(r1, d_Yt.p, nullptr);
        k_sum2<<<1, kThreads, 0, st>>>(m, d_fpart.p, d_gpart.p, d_sums.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(sums, d_sums.p, sizeof(sums), hipMemcpyDeviceToHost));
        const double ft = sums[0], gnorm = std::sqrt(sums[1]);
        if (ft < best_f) { best_f = ft; best_alpha = alpha; }   // the first of equal minima, as std::min_element
        if (ft < FY && gnorm > o.gradient_tolerance && gnorm > o.preconditioned_gradient_tolerance) { escaped = true; accepted = alpha; break; }
      }
      if (!escaped && best_f < FY) { retract(best_alpha); escaped = fallback = true; accepted = best_alpha; }
      if (!escaped) retract(0.0);   // the reference has augmented the rank already: Y keeps its zero row
      if ((rc = accept())) return rc;
      sm.escape_ms += ms_since(t_esc);
      log_level(hs.sweeps, FY, 0.0, lambda_min, rayleigh, accepted, fallback ? 1.0 : 0.0);
      rank = r1;
      if (!escaped) { end_state = THEIA_LAGRANGE_DUAL_END_ESCAPE_FAILED; break; }
    }
  }

  // ---- the solution; `rank` counts the zero row of a failed escape, as the reference's CurrentRank() does
  const int rounded = staircase ? rank > o.min_rank : rank > 3;
  with_rank<3, kMaxRank>(rank, [&](auto R) { k_solution<decltype(R)::value><<<view_grid, kThreads, 0, st>>>(m, rounded, d_Y.p, d_aa.p); });
  HIP_TRY(hipGetLastError());
  std::vector<double> aa(3 * (size_t)m), Yh((size_t)kStride * m);
  HIP_TRY(hipMemcpy(aa.data(), d_aa.p, sizeof(double) * aa.size(), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(Yh.data(), d_Y.p, sizeof(double) * Yh.size(), hipMemcpyDeviceToHost));
  double f_final = 0.0;
  if (end_state == THEIA_LAGRANGE_DUAL_END_BCM || end_state == THEIA_LAGRANGE_DUAL_END_CERTIFIED) {
    f_final = hs.f;
  } else {   // Y moved after the last BCM: f of what is returned
    gather(rank, d_Y.p, nullptr);
    k_sum2<<<1, kThreads, 0, st>>>(m, d_fpart.p, nullptr, d_sums.p);
    HIP_TRY(hipGetLastError());
    double sums[2];
    HIP_TRY(hipMemcpy(sums, d_sums.p, sizeof(sums), hipMemcpyDeviceToHost));
    f_final = sums[0];
  }
  for (int v = 0; v < n; ++v) {
    estimated_out[v] = idx[v] >= 0;
    if (idx[v] < 0) continue;
    for (int c = 0; c < 3; ++c) orientations_out[3 * (size_t)v + c] = aa[3 * (size_t)idx[v] + c];
  }
  if (y_out)
    for (int k = 0; k < rank; ++k)
      for (int i = 0; i < m; ++i)
        for (int c = 0; c < 3; ++c) y_out[(size_t)k * n3 + 3 * i + c] = Yh[(size_t)kStride * i + 3 * k + c];
  sm.total_iterations_num = hs.sweeps + 1;
  sm.sweeps = hs.sweeps;
  sm.final_rank = rank;
  sm.end_state = end_state;
  sm.num_levels = num_levels;
  sm.f = f_final;
  sm.total_ms = ms_since(t_start);
  *summary = sm;
  return 0;
}
