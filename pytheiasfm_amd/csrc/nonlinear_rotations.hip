// nonlinear_rotations.hip -- NonlinearRotationEstimator (global_pose_estimation/nonlinear_rotation_estimator.{h,cc},
// pairwise_rotation_error.{h,cc}; pybind sfm.cc:1782-1787): the Ceres Levenberg-Marquardt solve over PairwiseRotationError
// with a SoftL1 loss, on the device in FP64.  DESIGN.md 3.6i has the derivation.
//
// Per pair e = (i, j) the residual is r_e = log(R(w_j) R(w_i)' R(rel_e)') as an angle-axis vector: three
// ceres::AngleAxisToRotationMatrix and one ceres::RotationMatrixToAngleAxis (through the quaternion), with the small-angle
// branches of both.  Its two 3 x 3 Jacobians are the chain rule through the branch actually taken -- what Ceres' Jets give:
//   dR/dw_k      Rodrigues, R = c I + (1 - c) u u' + s [u]x, u = w / theta (theta^2 > eps), else I + [w]x
//   dE           dR_j,k (R_i' R_rel')  and  R_j (dR_i,k' R_rel')
//   dq           the quaternion of E by the trace branch (trace >= 0) or the largest-diagonal branch
//   dr           2 atan2(|v|, q0) v / |v| (|v|^2 > 0, with Ceres' sign handling for q0 < 0), else 2 v
// SoftLOneLoss(a) on s = |r|^2: rho'' < 0 everywhere, so Ceres' corrector scales residual and Jacobian by sqrt(rho').
//
// The LM loop is Ceres 2.2's TrustRegionMinimizer + LevenbergMarquardtStrategy on the dense normal
// equations of order 3m (m = the free views that have an edge):
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
#include "dense_cholesky.h"
#include "view_graph_device.h"

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <vector>

namespace thip {
namespace {

constexpr int kThreads = 256;
static_assert(kThreads == 64 * kViewsPerBlock, "k_column_norms, k_gradient: one wavefront per free view");
constexpr int kRec = 24;                        // doubles per edge record: J_i [3][3] | J_j [3][3] | r [3] | 3 unused
constexpr int kDefaultChunk = 4;                // LM iterations enqueued between two reads of the state
constexpr int kMaxChunk = 64;

struct NlState {
  int done, term, iterations, successful, unsuccessful, invalid;
  int invalid_run;       // consecutive invalid steps
  int step_successful;   // the last step was accepted (the gradient rule applies after successful steps only)
  int fresh;             // the iterate changed: k_linearise / k_gradient run, k_post takes the new gradient
  int trace_rows, pad0, pad1;
  double cost, initial_cost, gmax, x_norm, radius, decrease;
};

// ceres::AngleAxisToRotationMatrix, row-major, and what its derivative needs
struct AaCtx {
  double u[3], theta, c, s;
  bool big;
};

__device__ __forceinline__ void aa_rot(const double* w, AaCtx& a, double* R) {
  const double t2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
  a.big = t2 > DBL_EPSILON;
  if (a.big) {
    a.theta = sqrt(t2);
    const double wx = w[0] / a.theta, wy = w[1] / a.theta, wz = w[2] / a.theta;
    const double c = cos(a.theta), s = sin(a.theta);
    a.u[0] = wx; a.u[1] = wy; a.u[2] = wz; a.c = c; a.s = s;
    R[0] = c + wx * wx * (1.0 - c);      R[3] = wz * s + wx * wy * (1.0 - c);  R[6] = -wy * s + wx * wz * (1.0 - c);
    R[1] = wx * wy * (1.0 - c) - wz * s; R[4] = c + wy * wy * (1.0 - c);       R[7] = wx * s + wy * wz * (1.0 - c);
    R[2] = wy * s + wx * wz * (1.0 - c); R[5] = -wx * s + wy * wz * (1.0 - c); R[8] = c + wz * wz * (1.0 - c);
  } else {
    a.u[0] = a.u[1] = a.u[2] = 0.0; a.theta = 0.0; a.c = 1.0; a.s = 0.0;
    R[0] = 1.0; R[3] = w[2]; R[6] = -w[1];
    R[1] = -w[2]; R[4] = 1.0; R[7] = w[0];
    R[2] = w[1]; R[5] = -w[0]; R[8] = 1.0;
  }
}

// dR / dw_K of the branch aa_rot took
template <int K>
__device__ __forceinline__ void aa_rot_d(const AaCtx& a, double* D) {
  double v[3];   // the derivative of s u, the vector of the skew part
  if (a.big) {
    double du[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) du[i] = ((i == K ? 1.0 : 0.0) - a.u[i] * a.u[K]) / a.theta;
    const double dc = -a.s * a.u[K], ds = a.c * a.u[K], omc = 1.0 - a.c;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int q = 0; q < 3; ++q)
        D[3 * r + q] = ((r == q ? dc : 0.0) - dc * (a.u[r] * a.u[q])) + omc * (du[r] * a.u[q] + a.u[r] * du[q]);
#pragma unroll
    for (int i = 0; i < 3; ++i) v[i] = ds * a.u[i] + a.s * du[i];
  } else {
#pragma unroll
    for (int q = 0; q < 9; ++q) D[q] = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) v[i] = i == K ? 1.0 : 0.0;
  }
  D[1] -= v[2]; D[2] += v[1]; D[3] += v[2]; D[5] -= v[0]; D[6] -= v[1]; D[7] += v[0];
}

// ceres::RotationMatrixToAngleAxis (RotationMatrixToQuaternion, then QuaternionToAngleAxis) and what its derivative needs
struct LogCtx {
  int branch;   // 0: trace >= 0; 1 + i: the largest diagonal entry is i
  bool has_sin;
  double t, h, q[4], st, kf;
};

template <int I>
__device__ __forceinline__ void quat_diag(const double* E, LogCtx& L) {
  constexpr int J = (I + 1) % 3, K = (J + 1) % 3;
  L.t = sqrt(E[I * 3 + I] - E[J * 3 + J] - E[K * 3 + K] + 1.0);
  L.q[I + 1] = 0.5 * L.t;
  L.h = 0.5 / L.t;
  L.q[0] = (E[K * 3 + J] - E[J * 3 + K]) * L.h;
  L.q[J + 1] = (E[J * 3 + I] + E[I * 3 + J]) * L.h;
  L.q[K + 1] = (E[K * 3 + I] + E[I * 3 + K]) * L.h;
}
template <int I>
__device__ __forceinline__ void quat_diag_d(const double* E, const double* dE, const LogCtx& L, double* dq) {
  constexpr int J = (I + 1) % 3, K = (J + 1) % 3;
  const double dt = (dE[I * 3 + I] - dE[J * 3 + J] - dE[K * 3 + K]) / (2.0 * L.t);
  const double dh = -0.5 * dt / (L.t * L.t);
  dq[I + 1] = 0.5 * dt;
  dq[0] = (dE[K * 3 + J] - dE[J * 3 + K]) * L.h + (E[K * 3 + J] - E[J * 3 + K]) * dh;
  dq[J + 1] = (dE[J * 3 + I] + dE[I * 3 + J]) * L.h + (E[J * 3 + I] + E[I * 3 + J]) * dh;
  dq[K + 1] = (dE[K * 3 + I] + dE[I * 3 + K]) * L.h + (E[K * 3 + I] + E[I * 3 + K]) * dh;
}

__device__ __forceinline__ void log_rot(const double* E, LogCtx& L, double* r) {
  const double trace = E[0] + E[4] + E[8];
  if (trace >= 0.0) {
    L.branch = 0;
    L.t = sqrt(trace + 1.0);
    L.q[0] = 0.5 * L.t;
    L.h = 0.5 / L.t;
    L.q[1] = (E[7] - E[5]) * L.h; L.q[2] = (E[2] - E[6]) * L.h; L.q[3] = (E[3] - E[1]) * L.h;
  } else if (E[0] >= E[4] && E[0] >= E[8]) {   // i = 0 unless E11 > E00, then i = 2 if E22 > E[i][i]
    L.branch = 1; quat_diag<0>(E, L);
  } else if (E[4] > E[0] && E[4] >= E[8]) {
    L.branch = 2; quat_diag<1>(E, L);
  } else {
    L.branch = 3; quat_diag<2>(E, L);
  }
  const double s2 = L.q[1] * L.q[1] + L.q[2] * L.q[2] + L.q[3] * L.q[3];
  L.has_sin = s2 > 0.0;
  if (L.has_sin) {
    L.st = sqrt(s2);
    const double ct = L.q[0];
    const double two_theta = 2.0 * ((ct < 0.0) ? atan2(-L.st, -ct) : atan2(L.st, ct));
    L.kf = two_theta / L.st;
  } else {
    L.st = 0.0;
    L.kf = 2.0;
  }
  r[0] = L.q[1] * L.kf; r[1] = L.q[2] * L.kf; r[2] = L.q[3] * L.kf;
}

// dr for the matrix derivative dE, through the branches log_rot took
__device__ __forceinline__ void log_rot_d(const double* E, const double* dE, const LogCtx& L, double* dr) {
  double dq[4];
  if (L.branch == 0) {
    const double dt = ((dE[0] + dE[4]) + dE[8]) / (2.0 * L.t);
    const double dh = -0.5 * dt / (L.t * L.t);
    dq[0] = 0.5 * dt;
    dq[1] = (dE[7] - dE[5]) * L.h + (E[7] - E[5]) * dh;
    dq[2] = (dE[2] - dE[6]) * L.h + (E[2] - E[6]) * dh;
    dq[3] = (dE[3] - dE[1]) * L.h + (E[3] - E[1]) * dh;
  } else if (L.branch == 1) {
    quat_diag_d<0>(E, dE, L, dq);
  } else if (L.branch == 2) {
    quat_diag_d<1>(E, dE, L, dq);
  } else {
    quat_diag_d<2>(E, dE, L, dq);
  }
  if (L.has_sin) {
    const double ct = L.q[0];
    const double dst = ((L.q[1] * dq[1] + L.q[2] * dq[2]) + L.q[3] * dq[3]) / L.st;
    const double dtt = 2.0 * (ct * dst - L.st * dq[0]) / (L.st * L.st + ct * ct);
    const double dk = (dtt - L.kf * dst) / L.st;
    dr[0] = dq[1] * L.kf + L.q[1] * dk; dr[1] = dq[2] * L.kf + L.q[2] * dk; dr[2] = dq[3] * L.kf + L.q[3] * dk;
  } else {
    dr[0] = 2.0 * dq[1]; dr[1] = 2.0 * dq[2]; dr[2] = 2.0 * dq[3];
  }
}

// C = A B, C = A' B', all row-major 3 x 3
__device__ __forceinline__ void mul33(const double* A, const double* B, double* C) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) C[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
}
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
  mul33(v.Rj, v.M, v.Em);
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
    mul33(D, v.M, dE);
    log_rot_d(v.Em, dE, v.L, dr);
#pragma unroll
    for (int r = 0; r < 3; ++r) Jj[3 * r + K] = (dr[r] * v.sr) * sj[K];
  }
  if (free_i) {
    aa_rot_d<K>(v.ci, D);
    mul33_tt(D, v.Rrel, N);
    mul33(v.Rj, N, dE);
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

// The first linearisation ran with scale = 1; one wavefront per free view sums the squares of its three columns over its
// incident edges (lane l takes edges l, l + 64, .. in order, then the butterfly) and writes scale = 1 / (1 + |column|).
__global__ __launch_bounds__(kThreads) void k_column_norms(ViewGraphLists vg, const double* __restrict__ rec,
                                                           double* __restrict__ scale) {
  const int v = blockIdx.x * kViewsPerBlock + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (v >= vg.m) return;   // wave-uniform
  double s[3] = {0.0, 0.0, 0.0};
  for_each_incident_edge(vg, v, lane, [&](int e, bool plus) {
    const double* J = rec + kRec * (size_t)e + 9 * (int)plus;
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] += (J[c] * J[c] + J[3 + c] * J[3 + c]) + J[6 + c] * J[6 + c];
  });
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double t = wave_sum_butterfly(s[c]);
    if (lane == 0) scale[3 * (size_t)v + c] = 1.0 / (1.0 + sqrt(t));
  }
}

// g = Js' r, one wavefront per free view as above; part_g[block] = max |g / scale| over the workgroup's views (the
// gradient of the unscaled problem, which the gradient tolerance is about).
__global__ __launch_bounds__(kThreads) void k_gradient(ViewGraphLists vg, const double* __restrict__ rec,
                                                       const double* __restrict__ scale, double* __restrict__ g,
                                                       double* __restrict__ part_g, const NlState* __restrict__ st) {
  __shared__ double red[kViewsPerBlock];
  if (st->done || !st->fresh) return;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int v = blockIdx.x * kViewsPerBlock + wv;
  double gm = 0.0;
  if (v < vg.m) {   // wave-uniform
    double s[3] = {0.0, 0.0, 0.0};
    for_each_incident_edge(vg, v, lane, [&](int e, bool plus) {
      const double* R = rec + kRec * (size_t)e;
      const double* J = R + 9 * (int)plus;
#pragma unroll
      for (int c = 0; c < 3; ++c) s[c] += (J[c] * R[18] + J[3 + c] * R[19]) + J[6 + c] * R[20];
    });
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double t = wave_sum_butterfly(s[c]);
      if (lane == 0) g[3 * (size_t)v + c] = t;
      gm = fmax(gm, fabs(t / scale[3 * (size_t)v + c]));
    }
  }
  if (lane == 0) red[wv] = gm;
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = red[0];
    for (int k = 1; k < kViewsPerBlock; ++k) a = fmax(a, red[k]);
    part_g[blockIdx.x] = a;
  }
}

__device__ __forceinline__ void trace_row(double* trace, int capacity_rows, NlState* st, double cost, double gmax,
                                          double step, double radius, int accepted) {
  if (st->trace_rows < capacity_rows) {
    double* t = trace + 5 * (size_t)st->trace_rows;
    t[0] = cost; t[1] = gmax; t[2] = step; t[3] = radius; t[4] = (double)accepted;
  }
  st->trace_rows += 1;
}

// One workgroup, after every k_decide and once at the start (init = 1).  When the iterate is fresh: the gradient max norm
// of the new linearisation (at the start also the cost, |x| and trace row 0) goes into the state and the trace.  Then
// the rules that end the loop between two iterations, in Ceres' order: at the start the gradient tolerance, then the cap;
// afterwards the cap, the gradient tolerance (after a successful step only), the radius floor.
__global__ __launch_bounds__(kThreads) void k_post(int init, int m, const int* __restrict__ free_view,
                                                   const double* __restrict__ x, const double* __restrict__ part_cost, int nbE,
                                                   const double* __restrict__ part_g, int nbV, int max_iterations,
                                                   double gradient_tolerance, double* __restrict__ trace,
                                                   int capacity_rows, int term_gradient, int term_cap, int term_radius,
                                                   NlState* __restrict__ st) {
  __shared__ double red[kThreads];
  __shared__ int flags[2];
  if (threadIdx.x == 0) { flags[0] = st->done; flags[1] = st->fresh; }
  __syncthreads();
  if (flags[0]) return;
  const bool fresh = flags[1] != 0;
  double gmax = 0.0, cost = 0.0, xn = 0.0;
  if (fresh) {
    double a = 0.0;
    for (int k = threadIdx.x; k < nbV; k += kThreads) a = fmax(a, part_g[k]);
    red[threadIdx.x] = a;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
      __syncthreads();
    }
    gmax = red[0];
    __syncthreads();
    if (init) {
      double q = 0.0;
      for (int k = threadIdx.x; k < m; k += kThreads) {
        const double* w = x + 3 * (size_t)free_view[k];
        q += (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
      }
      cost = block_sum_column<kThreads>(part_cost, nbE, 1, 0, red);
      xn = block_sum<kThreads>(q, red);
    }
  }
  if (threadIdx.x != 0) return;
  if (fresh) {
    st->gmax = gmax;
    if (init) {
      st->cost = st->initial_cost = 0.5 * cost;
      st->x_norm = sqrt(xn);
      trace_row(trace, capacity_rows, st, st->cost, gmax, 0.0, st->radius, 1);
    } else if (st->trace_rows - 1 < capacity_rows) {
      trace[5 * (size_t)(st->trace_rows - 1) + 1] = gmax;
    }
    st->fresh = 0;
  }
  const bool grad = st->step_successful && st->gmax <= gradient_tolerance;
  const bool cap = st->iterations >= max_iterations;
  if (init && grad) { st->done = 1; st->term = term_gradient; }
  else if (cap) { st->done = 1; st->term = term_cap; }
  else if (grad) { st->done = 1; st->term = term_gradient; }
  else if (st->radius <= 1e-32) { st->done = 1; st->term = term_radius; }
}

// The lower triangle of Js'Js + D into the cleared array (row-major, leading dimension lda), D = clamp(diag(Js'Js), 1e-6,
// 1e32) / radius, and g into row 3m, the factorisation's right-hand-side row:
//   thread t < m       : free view t -- its 3 x 3 diagonal block, sum of J' J over its incident edges, and its part of g
//   thread t = m + p   : pair p = (a > b) -- block (a, b) = sum of J_a' J_b over the pair's edges
__global__ __launch_bounds__(kThreads) void k_assemble(ViewGraphLists vg, int lda, const double* __restrict__ rec,
                                                       const double* __restrict__ g, double* __restrict__ A,
                                                       const NlState* __restrict__ st) {
  if (st->done) return;
  const int t = blockIdx.x * kThreads + threadIdx.x, m = vg.m;
  double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (t < m) {
    for (int k = vg.inc_off[t]; k < vg.inc_off[t + 1]; ++k) {
      const double* J = rec + kRec * (size_t)(vg.inc[k] >> 1) + 9 * (vg.inc[k] & 1);
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) acc[3 * r + c] += (J[r] * J[c] + J[3 + r] * J[3 + c]) + J[6 + r] * J[6 + c];
    }
    const double radius = st->radius;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < r; ++c) A[(size_t)(3 * t + r) * lda + 3 * t + c] = acc[3 * r + c];
      const double d = acc[4 * r];
      A[(size_t)(3 * t + r) * lda + 3 * t + r] = d + fmin(fmax(d, 1e-6), 1e32) / radius;
      A[(size_t)(3 * m) * lda + 3 * t + r] = g[3 * (size_t)t + r];
    }
  } else if (t < m + vg.P) {
    const int p = t - m;
    const int2 rc = vg.pair_rc[p];
    for (int k = vg.pair_off[p]; k < vg.pair_off[p + 1]; ++k) {
      const int e = vg.pair_edge[k];
      const bool second_is_row = vg.idx[vg.edges[e].y] == rc.x;
      const double* Ja = rec + kRec * (size_t)e + (second_is_row ? 9 : 0);
      const double* Jb = rec + kRec * (size_t)e + (second_is_row ? 0 : 9);
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[3 * r + c] += (Ja[r] * Jb[c] + Ja[3 + r] * Jb[3 + c]) + Ja[6 + r] * Jb[6 + c];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) A[(size_t)(3 * rc.x + r) * lda + 3 * rc.y + c] = acc[3 * r + c];
  }
}

// One lane per free view: the candidate xc = x - scale * y, and the blocks' sums of |x - xc|^2 and |xc|^2.
__global__ __launch_bounds__(kThreads) void k_step(int m, const int* __restrict__ free_view, const double* __restrict__ x,
                                                   const double* __restrict__ scale, const double* __restrict__ y,
                                                   double* __restrict__ xc, double* __restrict__ part,
                                                   const NlState* __restrict__ st) {
  __shared__ double red[kThreads];
  if (st->done) return;
  const int t = blockIdx.x * kThreads + threadIdx.x;
  double ss = 0.0, nn = 0.0;
  if (t < m) {
    const size_t v3 = 3 * (size_t)free_view[t];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double xo = x[v3 + k];
      const double xn = xo - y[3 * (size_t)t + k] * scale[3 * (size_t)t + k];
      xc[v3 + k] = xn;
      const double d = xo - xn;
      ss += d * d; nn += xn * xn;
    }
  }
  const double s0 = block_sum<kThreads>(ss, red), s1 = block_sum<kThreads>(nn, red);
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = s0; part[2 * blockIdx.x + 1] = s1; }
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

struct DecideArgs {
  int nbE, nbM, n3_views;   // blocks of k_candidate, blocks of k_step, 3 * num_views
  int capacity_rows, term_parameter, term_function, term_failure;
  double function_tolerance, parameter_tolerance, max_radius;
};

// One workgroup: sums the blocks' partials in block order, then thread 0 runs one pass of TrustRegionMinimizer's loop
// body in Ceres' order: invalid step (a failed factorisation, a non-finite step, a model cost change that is not
// positive), parameter tolerance, function tolerance, rho > 1e-3, radius update.  On acceptance the workgroup copies the
// candidate over the iterate and marks it fresh.
__global__ __launch_bounds__(kThreads) void k_decide(DecideArgs a, const double* __restrict__ part_cand,
                                                     const double* __restrict__ part_step, double* __restrict__ fail_flag,
                                                     double* __restrict__ x, const double* __restrict__ xc,
                                                     double* __restrict__ trace, NlState* __restrict__ st) {
  __shared__ double red[kThreads];
  __shared__ int flags[2];
  if (threadIdx.x == 0) { flags[0] = st->done; flags[1] = 0; }
  __syncthreads();
  if (flags[0]) return;
  double sum[4];
  for (int c = 0; c < 2; ++c) sum[c] = block_sum_column<kThreads>(part_cand, a.nbE, 2, c, red);
  for (int c = 0; c < 2; ++c) sum[2 + c] = block_sum_column<kThreads>(part_step, a.nbM, 2, c, red);
  if (threadIdx.x == 0) {
    const double failed = *fail_flag;
    *fail_flag = 0.0;
    st->iterations += 1;
    const double model = sum[1], step_sq = sum[2];
    const bool ok = failed == 0.0 && isfinite(step_sq) && isfinite(model) && model > 0.0;
    if (!ok) {
      st->invalid += 1;
      st->invalid_run += 1;
      if (st->invalid_run >= 5) {
        st->done = 1; st->term = a.term_failure;
      } else {
        st->radius /= st->decrease; st->decrease *= 2.0; st->step_successful = 0;
        trace_row(trace, a.capacity_rows, st, st->cost, st->gmax, 0.0, st->radius, 0);
      }
    } else {
      st->invalid_run = 0;
      double cand = 0.5 * sum[0];
      if (!isfinite(cand)) cand = DBL_MAX;
      const double step_norm = sqrt(step_sq);
      const double change = st->cost - cand;
      if (step_norm <= a.parameter_tolerance * (st->x_norm + a.parameter_tolerance)) {
        trace_row(trace, a.capacity_rows, st, cand, st->gmax, step_norm, st->radius, 0);
        st->done = 1; st->term = a.term_parameter;
      } else if (fabs(change) <= a.function_tolerance * st->cost) {
        trace_row(trace, a.capacity_rows, st, cand, st->gmax, step_norm, st->radius, 0);
        st->done = 1; st->term = a.term_function;
      } else {
        const double rho = change / model;
        if (rho > 1e-3) {
          const double w = 2.0 * rho - 1.0;
          st->cost = cand;
          st->x_norm = sqrt(sum[3]);
          st->radius = fmin(a.max_radius, st->radius / fmax(1.0 / 3.0, 1.0 - w * w * w));
          st->decrease = 2.0; st->step_successful = 1; st->successful += 1; st->fresh = 1;
          trace_row(trace, a.capacity_rows, st, cand, st->gmax, step_norm, st->radius, 1);   // k_post: the new gradient
          flags[1] = 1;
        } else {
          st->radius /= st->decrease; st->decrease *= 2.0; st->step_successful = 0; st->unsuccessful += 1;
          trace_row(trace, a.capacity_rows, st, cand, st->gmax, step_norm, st->radius, 0);
        }
      }
    }
  }
  __syncthreads();
  if (flags[1])
    for (int k = threadIdx.x; k < a.n3_views; k += kThreads) x[k] = xc[k];
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

bool positive_finite(double v) { return v > 0.0 && std::isfinite(v); }
bool nonnegative_finite(double v) { return v >= 0.0 && std::isfinite(v); }

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
  hs.radius = 1e4; hs.decrease = 2.0; hs.fresh = 1; hs.step_successful = 1;
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
  const char* chunk_env = getenv("THEIA_HIP_LM_CHUNK");
  const int chunk_size = std::max(1, std::min(chunk_env ? atoi(chunk_env) : kDefaultChunk, kMaxChunk));
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
