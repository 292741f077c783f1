// alignment.hip -- reconstruction alignment (sfm/transformation/): theia_hip_align_point_clouds (the weighted Umeyama of
// align_point_clouds.cc:56-150 for a batch of point-cloud pairs), theia_hip_transform_reconstruction
// (transform_reconstruction.cc:48-94 on flat arrays) and theia_hip_align_rotations (align_rotations.cc:127-156).  The per-thread
// arithmetic is alignment_device.h and rotation_derivatives.h; this file must be compiled without FMA contraction (build.sh's
// default).  DESIGN.md 3.6t.
//
// k_umeyama<WAVES>   one team of WAVES wavefronts per problem: WAVES = 1, four problems per 256-lane workgroup, for problems of
//                    up to THEIA_ALIGN_WAVE_MAX_POINTS points (the host lists them); WAVES = 4, one workgroup per problem,
//                    for the larger ones.  Two passes over the problem's points, as the reference makes them: (1) weight sum
//                    and the weighted sums of left and right -> centroids; (2) sigma and the nine entries of the centred
//                    cross-correlation.  Every sum has ONE owner and ONE order: lane l of the team adds the points l, l + T,
//                    l + 2T, ... (T = 64 WAVES) in that order, the wave adds its lanes by the XOR butterfly (wave_reduce.h), and
//                    (WAVES = 4) every lane adds the four wave sums from LDS in wave order.  No atomics; the bytes of a result do
//                    not depend on the launch, on the other problems of the batch or on the run.  Lane 0 of the team finishes
//                    with umeyama_finish().
// k_transform        one lane per camera or point, 256 per workgroup; a masked-out entry is neither read nor written.
// k_align_rotations  AlignRotations (align_rotations.cc:127-156): the whole Levenberg-Marquardt solve over one 3-parameter
//                    block in ONE workgroup and one launch.  Lanes stride over the rotations; a pass over them sums the cost,
//                    J'r and the lower triangle of J'J (ten numbers) by team_sum<4> -- every lane then holds the same bits, so
//                    every lane runs the 3 x 3 solve and Ceres' rules (lm_rules.h) on its own copy of the state and the
//                    workgroup's control flow stays uniform without a broadcast; lane 0 writes the trace and the result.
//                    The residual gt_i - log(R_i R(w)) and its Jacobian -dlog(R_i R(w)) (R_i dR/dw_k) use the closed forms of
//                    rotation_derivatives.h (those of the NONLINEAR rotation stage).  R_i is formed once, into `Ru`.
#include "alignment_device.h"
#include "lm_rules.h"
#include "rotation_derivatives.h"
#include "wave_reduce.h"
#include "device_util.h"

#include <cmath>
#include <vector>

namespace thip {
namespace {

constexpr int kThreads = 256;
constexpr int kWaveMax = THEIA_ALIGN_WAVE_MAX_POINTS;

// sum over the team; every lane of every wave of the team takes part
template <int WAVES>
__device__ __forceinline__ double team_sum(double v, double* red /* [WAVES], LDS */) {
  v = wave_sum_butterfly(v);
  if (WAVES == 1) return v;
  const int wave = threadIdx.x >> 6;
  __syncthreads();   // the previous sum's readers are done with red
  if ((threadIdx.x & 63) == 0) red[wave] = v;
  __syncthreads();
  double s = red[0];
  for (int w = 1; w < WAVES; ++w) s += red[w];
  return s;
}

template <int WAVES>
__global__ __launch_bounds__(kThreads) void k_umeyama(int count, const int* __restrict__ problems,
                                                      const long long* __restrict__ offsets, const double* __restrict__ left,
                                                      const double* __restrict__ right, const double* __restrict__ weights,
                                                      double* __restrict__ out /* [P][13] */, int* __restrict__ status) {
  __shared__ double red[4];
  constexpr int T = 64 * WAVES;
  const int team = WAVES == 1 ? (int)(blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6)) : (int)blockIdx.x;
  if (team >= count) return;   // a whole wave (WAVES == 1) or a whole workgroup leaves together
  const int lane = WAVES == 1 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
  const int p = problems[team];
  const long long i0 = offsets[p], n = offsets[p + 1] - i0;
  const double* L = left + 3 * i0;
  const double* Rr = right + 3 * i0;
  const double* W = weights ? weights + i0 : nullptr;

  double acc[10];
  for (int k = 0; k < 7; ++k) acc[k] = 0.0;
  for (long long i = lane; i < n; i += T) {
    const double w = W ? W[i] : 1.0;
    acc[0] += w;
    for (int k = 0; k < 3; ++k) { acc[1 + k] += L[3 * i + k] * w; acc[4 + k] += Rr[3 * i + k] * w; }
  }
  for (int k = 0; k < 7; ++k) acc[k] = team_sum<WAVES>(acc[k], red);
  const double wsum = acc[0];
  double lc[3], rc[3];
  for (int k = 0; k < 3; ++k) { lc[k] = acc[1 + k] / wsum; rc[k] = acc[4 + k] / wsum; }

  for (int k = 0; k < 10; ++k) acc[k] = 0.0;
  for (long long i = lane; i < n; i += T) {
    const double w = W ? W[i] : 1.0;
    double dl[3], dr[3];
    for (int k = 0; k < 3; ++k) { dl[k] = L[3 * i + k] - lc[k]; dr[k] = Rr[3 * i + k] - rc[k]; }
    acc[0] += ((dl[0] * dl[0] + dl[1] * dl[1]) + dl[2] * dl[2]) * w;
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) acc[1 + 3 * a + b] += (w * dl[a]) * dr[b];
  }
  for (int k = 0; k < 10; ++k) acc[k] = team_sum<WAVES>(acc[k], red);
  if (lane != 0) return;
  const double sigma = acc[0] / wsum;
  double cc[9];
  for (int k = 0; k < 9; ++k) cc[k] = acc[1 + k] / wsum;
  double* o = out + (size_t)p * 13;
  status[p] = rsc::umeyama_finish(lc, rc, sigma, cc, o, o + 9, o + 12);
}

struct Sim { double R[9], t[3], s; };

__global__ __launch_bounds__(kThreads) void k_transform(int num_cameras, double* __restrict__ cameras,
                                                        const uint8_t* __restrict__ cam_mask, long long num_points,
                                                        double* __restrict__ points, const uint8_t* __restrict__ pt_mask, Sim T) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i < num_cameras) {
    if (cam_mask && !cam_mask[i]) return;
    double cam[6];
    for (int k = 0; k < 6; ++k) cam[k] = cameras[6 * i + k];
    rsc::transform_camera(T.R, T.t, T.s, cam);
    for (int k = 0; k < 6; ++k) cameras[6 * i + k] = cam[k];
    return;
  }
  const long long j = i - num_cameras;
  if (j >= num_points) return;
  if (pt_mask && !pt_mask[j]) return;
  double4* P4 = reinterpret_cast<double4*>(points);   // hipMalloc's alignment; one 32 B load and store per point
  const double4 v = P4[j];
  double pt[4] = {v.x, v.y, v.z, v.w};
  rsc::transform_point(T.R, T.t, T.s, pt);
  P4[j] = make_double4(pt[0], pt[1], pt[2], pt[3]);
}

// ---- AlignRotations
struct AlignRotState {
  int iterations, successful, unsuccessful, invalid, term, trace_rows;
  double initial_cost, cost, radius, gmax, w[3];
};
// ceres::Solver::Options as align_rotations.cc:147-149 leaves them (Ceres 2.2)
constexpr int kArMaxIterations = 50;
constexpr double kArFunctionTolerance = 0.0, kArGradientTolerance = 1e-10, kArParameterTolerance = 1e-8, kArMaxRadius = 1e16;

struct ArSums { double cost, g[3], H[6]; };   // sum |r|^2 / 2, J'r, the packed lower triangle of J'J

// one pass over the rotations at w: the cost alone (JAC = false) or with J'r and J'J
template <bool JAC>
__device__ __forceinline__ void ar_pass(int n, const double* __restrict__ gt, const double* __restrict__ Ru, const double* w,
                                        ArSums& out, double* red) {
  AaCtx cw;
  double Rw[9], D[3][9];
  aa_rot(w, cw, Rw);
  if (JAC) { aa_rot_d<0>(cw, D[0]); aa_rot_d<1>(cw, D[1]); aa_rot_d<2>(cw, D[2]); }
  double acc[10];
  for (int k = 0; k < 10; ++k) acc[k] = 0.0;
  for (int i = threadIdx.x; i < n; i += kThreads) {
    double R[9], M[9], a[3], r[3];
    for (int k = 0; k < 9; ++k) R[k] = Ru[9 * (size_t)i + k];
    rsc::matmul3(R, Rw, M);
    LogCtx L;
    log_rot(M, L, a);
    for (int k = 0; k < 3; ++k) r[k] = gt[3 * (size_t)i + k] - a[k];
    acc[0] += (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
    if (JAC) {
      double J[9];   // row-major 3 x 3: J[3 r + k] = d residual_r / d w_k
      for (int k = 0; k < 3; ++k) {
        double dM[9], dr[3];
        rsc::matmul3(R, D[k], dM);
        log_rot_d(M, dM, L, dr);
        for (int q = 0; q < 3; ++q) J[3 * q + k] = -dr[q];
      }
      for (int k = 0; k < 3; ++k) acc[1 + k] += (J[k] * r[0] + J[3 + k] * r[1]) + J[6 + k] * r[2];
      for (int a2 = 0; a2 < 3; ++a2)
        for (int b = 0; b <= a2; ++b) acc[4 + lm::tri(a2, b)] += (J[a2] * J[b] + J[3 + a2] * J[3 + b]) + J[6 + a2] * J[6 + b];
    }
  }
  out.cost = 0.5 * team_sum<4>(acc[0], red);
  if (JAC) {
    for (int k = 0; k < 3; ++k) out.g[k] = team_sum<4>(acc[1 + k], red);
    for (int k = 0; k < 6; ++k) out.H[k] = team_sum<4>(acc[4 + k], red);
  }
}

// (H + diag(d)) y = g by Cholesky in registers, H packed lower; false on a pivot that is not positive or a non-finite y
__device__ __forceinline__ bool ar_solve3(const double* H, const double* d, const double* g, double* y) {
  const double a00 = H[0] + d[0], a10 = H[1], a11 = H[2] + d[1], a20 = H[3], a21 = H[4], a22 = H[5] + d[2];
  if (!(a00 > 0.0)) return false;
  const double l00 = sqrt(a00), l10 = a10 / l00, l20 = a20 / l00;
  const double p11 = a11 - l10 * l10;
  if (!(p11 > 0.0)) return false;
  const double l11 = sqrt(p11), l21 = (a21 - l20 * l10) / l11;
  const double p22 = a22 - l20 * l20 - l21 * l21;
  if (!(p22 > 0.0)) return false;
  const double l22 = sqrt(p22);
  const double z0 = g[0] / l00, z1 = (g[1] - l10 * z0) / l11, z2 = (g[2] - l20 * z0 - l21 * z1) / l22;
  y[2] = z2 / l22;
  y[1] = (z1 - l21 * y[2]) / l11;
  y[0] = (z0 - l10 * y[1] - l20 * y[2]) / l00;
  return isfinite(y[0]) && isfinite(y[1]) && isfinite(y[2]);
}

__device__ __forceinline__ void ar_trace(double* trace, int capacity_rows, int& rows, double cost, double gmax, double step_norm,
                                         double radius, int accepted) {
  if (threadIdx.x == 0 && trace && rows < capacity_rows) {
    double* t = trace + 5 * (size_t)rows;
    t[0] = cost; t[1] = gmax; t[2] = step_norm; t[3] = radius; t[4] = (double)accepted;
  }
  rows += 1;
}

__global__ __launch_bounds__(kThreads) void k_align_rotations(int n, const double* __restrict__ gt, double* __restrict__ rot,
                                                              double* __restrict__ Ru, double* __restrict__ trace,
                                                              int capacity_rows, AlignRotState* __restrict__ out) {
  __shared__ double red[4];
  for (int i = threadIdx.x; i < n; i += kThreads) rsc::angle_axis_to_rot(rot + 3 * (size_t)i, Ru + 9 * (size_t)i);
  // (each lane reads back only the rows of Ru it wrote: the stride is the same in every pass)
  double w[3] = {0.0, 0.0, 0.0}, scale[3], gs[3], Hs[6];
  ArSums S;
  ar_pass<true>(n, gt, Ru, w, S, red);
  for (int k = 0; k < 3; ++k) scale[k] = lm::jacobi_scale(S.H[lm::tri(k, k)]);
  double cost = S.cost, x_norm = 0.0;
  double gmax = fmax(fabs(S.g[0]), fmax(fabs(S.g[1]), fabs(S.g[2])));
  const double initial_cost = cost;
  lm::TrustRegion tr;
  int iterations = 0, successful = 0, unsuccessful = 0, invalid = 0, rows = 0, term = 0;
  ar_trace(trace, capacity_rows, rows, cost, gmax, 0.0, tr.radius, 1);
  bool fresh = true;
  while (true) {
    if (iterations >= kArMaxIterations) { term = THEIA_ROTATION_TERM_MAX_ITERATIONS; break; }
    if (lm::gradient_rule(tr, gmax, kArGradientTolerance)) { term = THEIA_ROTATION_TERM_GRADIENT_TOLERANCE; break; }
    if (lm::radius_floor(tr)) { term = THEIA_ROTATION_TERM_MIN_RADIUS; break; }
    iterations += 1;
    if (fresh) {   // the Jacobi-scaled system of the iterate
      for (int k = 0; k < 3; ++k) gs[k] = S.g[k] * scale[k];
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b <= a; ++b) Hs[lm::tri(a, b)] = (S.H[lm::tri(a, b)] * scale[a]) * scale[b];
      fresh = false;
    }
    double d[3], y[3];
    for (int k = 0; k < 3; ++k) d[k] = lm::lm_diagonal(Hs[lm::tri(k, k)], tr.radius);
    bool ok = ar_solve3(Hs, d, gs, y);
    double model = 0.0;
    if (ok) {
      model = lm::model_cost_change<3>(Hs, gs, y);
      ok = isfinite(model) && model > 0.0;
    }
    if (!ok) {
      invalid += 1;
      if (!lm::invalid_step(tr)) { term = THEIA_ROTATION_TERM_FAILURE; break; }
      ar_trace(trace, capacity_rows, rows, cost, gmax, 0.0, tr.radius, 0);
      continue;
    }
    lm::valid_step(tr);
    double delta[3], wc[3];
    for (int k = 0; k < 3; ++k) { delta[k] = -(y[k] * scale[k]); wc[k] = w[k] + delta[k]; }
    ArSums C;
    ar_pass<false>(n, gt, Ru, wc, C, red);
    double cand = C.cost;
    if (!isfinite(cand)) cand = DBL_MAX;
    const double step_norm = sqrt((delta[0] * delta[0] + delta[1] * delta[1]) + delta[2] * delta[2]);
    if (lm::parameter_rule(step_norm, x_norm, kArParameterTolerance)) {
      ar_trace(trace, capacity_rows, rows, cand, gmax, step_norm, tr.radius, 0);
      term = THEIA_ROTATION_TERM_PARAMETER_TOLERANCE; break;
    }
    if (lm::function_rule(cost, cand, kArFunctionTolerance)) {
      ar_trace(trace, capacity_rows, rows, cand, gmax, step_norm, tr.radius, 0);
      term = THEIA_ROTATION_TERM_FUNCTION_TOLERANCE; break;
    }
    const double rho = (cost - cand) / model;
    if (lm::step_accepted(rho)) {
      for (int k = 0; k < 3; ++k) w[k] = wc[k];
      x_norm = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
      ar_pass<true>(n, gt, Ru, w, S, red);
      cost = S.cost;
      gmax = fmax(fabs(S.g[0]), fmax(fabs(S.g[1]), fabs(S.g[2])));
      lm::accept(tr, rho, kArMaxRadius);
      successful += 1; fresh = true;
      ar_trace(trace, capacity_rows, rows, cost, gmax, step_norm, tr.radius, 1);
    } else {
      lm::shrink(tr); unsuccessful += 1;
      ar_trace(trace, capacity_rows, rows, cand, gmax, step_norm, tr.radius, 0);
    }
  }
  if (term == THEIA_ROTATION_TERM_FAILURE) { w[0] = 0.0; w[1] = 0.0; w[2] = 0.0; }   // Ceres leaves the block as it was passed in
  // ApplyRotationTransformation (:100-123)
  double Rw[9];
  rsc::angle_axis_to_rot(w, Rw);
  for (int i = threadIdx.x; i < n; i += kThreads) {
    double R[9], M[9];
    for (int k = 0; k < 9; ++k) R[k] = Ru[9 * (size_t)i + k];
    rsc::matmul3(R, Rw, M);
    rsc::rot_to_angle_axis(M, rot + 3 * (size_t)i);
  }
  if (threadIdx.x == 0) {
    out->iterations = iterations; out->successful = successful; out->unsuccessful = unsuccessful; out->invalid = invalid;
    out->term = term; out->trace_rows = rows;
    out->initial_cost = initial_cost; out->cost = cost; out->radius = tr.radius; out->gmax = gmax;
    out->w[0] = w[0]; out->w[1] = w[1]; out->w[2] = w[2];
  }
}

// device events around a call's kernels (only when the caller asks for timings)
struct KernelClock {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  bool on = false;
  ~KernelClock() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
  hipError_t start(bool want) {
    on = want;
    if (!on) return hipSuccess;
    hipError_t r = hipEventCreate(&e0);
    if (r == hipSuccess) r = hipEventCreate(&e1);
    if (r == hipSuccess) r = hipEventRecord(e0, nullptr);
    return r;
  }
  hipError_t stop(float* ms) {
    *ms = 0.f;
    if (!on) return hipSuccess;
    hipError_t r = hipEventRecord(e1, nullptr);
    if (r == hipSuccess) r = hipEventSynchronize(e1);
    if (r == hipSuccess) r = hipEventElapsedTime(ms, e0, e1);
    return r;
  }
};

}  // namespace
}  // namespace thip

using namespace thip;

extern "C" int theia_hip_align_point_clouds(int32_t num_problems, const int64_t* offsets, const double* left, const double* right,
                                            const double* weights, double* rotation, double* translation, double* scale,
                                            int32_t* status, double* timings_ms) {
  const auto t_call = std::chrono::steady_clock::now();
  if (num_problems < 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "negative problem count");
  if (num_problems == 0) {
    if (timings_ms) { timings_ms[0] = 0.0; timings_ms[1] = ms_since(t_call); }
    return 0;
  }
  if (!offsets || !left || !right || !rotation || !translation || !scale || !status)
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null array");
  if (offsets[0] != 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "offsets[0] must be 0");
  std::vector<int> small_list, large_list;
  for (int p = 0; p < num_problems; ++p) {
    const int64_t i0 = offsets[p], i1 = offsets[p + 1];
    if (i1 < i0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "problem %d: decreasing offsets", p);
    if (i1 == i0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "problem %d has no points", p);
    double wsum = 0.0;
    for (int64_t i = i0; i < i1; ++i) {
      for (int k = 0; k < 3; ++k)
        if (!std::isfinite(left[3 * i + k]) || !std::isfinite(right[3 * i + k]))
          return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "problem %d: non-finite coordinate at point %lld", p, (long long)(i - i0));
      if (weights) {
        if (!std::isfinite(weights[i]))
          return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "problem %d: non-finite weight at point %lld", p, (long long)(i - i0));
        if (!(weights[i] >= 0.0))
          return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "The point weight must be greater or equal to zero.");
        wsum += weights[i];
      } else {
        wsum += 1.0;
      }
    }
    if (!(wsum > 0.0)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "The sum of weights must be greater than zero.");
    (i1 - i0 <= kWaveMax ? small_list : large_list).push_back(p);
  }

  int rc = ensure_device();
  if (rc) return rc;
  const size_t total = (size_t)offsets[num_problems], P = (size_t)num_problems;
  const size_t ns = small_list.size(), nl = large_list.size();
  DevBuf<long long> d_off;
  DevBuf<double> d_left, d_right, d_w, d_out;
  DevBuf<int> d_small, d_large, d_status;
  static_assert(sizeof(long long) == sizeof(int64_t), "offsets");
  if ((rc = d_off.up(offsets, P + 1)) || (rc = d_left.up(left, 3 * total)) || (rc = d_right.up(right, 3 * total)) ||
      (weights && (rc = d_w.up(weights, total))) || (rc = d_out.alloc(13 * P)) || (rc = d_status.alloc(P)) ||
      (rc = d_small.up(small_list.data(), ns)) || (rc = d_large.up(large_list.data(), nl)))
    return rc;
  KernelClock clk;
  HIP_TRY(clk.start(timings_ms != nullptr));
  if (ns)
    k_umeyama<1><<<grid_of(ns, kThreads / 64), kThreads>>>((int)ns, d_small.p, d_off.p, d_left.p, d_right.p, d_w.p, d_out.p, d_status.p);
  if (nl)
    k_umeyama<4><<<(unsigned)nl, kThreads>>>((int)nl, d_large.p, d_off.p, d_left.p, d_right.p, d_w.p, d_out.p, d_status.p);
  HIP_TRY(hipGetLastError());
  float kernel_ms = 0.f;
  HIP_TRY(clk.stop(&kernel_ms));
  std::vector<double> h_out(13 * P);
  std::vector<int> h_status(P);
  HIP_TRY(hipMemcpy(h_out.data(), d_out.p, sizeof(double) * 13 * P, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h_status.data(), d_status.p, sizeof(int) * P, hipMemcpyDeviceToHost));
  for (size_t p = 0; p < P; ++p) {
    for (int k = 0; k < 9; ++k) rotation[9 * p + k] = h_out[13 * p + k];
    for (int k = 0; k < 3; ++k) translation[3 * p + k] = h_out[13 * p + 9 + k];
    scale[p] = h_out[13 * p + 12];
    status[p] = h_status[p];
  }
  if (timings_ms) { timings_ms[0] = kernel_ms; timings_ms[1] = ms_since(t_call); }
  return 0;
}

extern "C" int theia_hip_transform_reconstruction(int32_t num_cameras, double* cameras, const uint8_t* camera_estimated,
                                                  int64_t num_points, double* points, const uint8_t* point_estimated,
                                                  const double* rotation, const double* translation, double scale,
                                                  double* timings_ms) {
  const auto t_call = std::chrono::steady_clock::now();
  if (num_cameras < 0 || num_points < 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "negative count");
  if ((num_cameras > 0 && !cameras) || (num_points > 0 && !points)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null array");
  if (!rotation || !translation) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null transformation");
  Sim T;
  for (int k = 0; k < 9; ++k) T.R[k] = rotation[k];
  for (int k = 0; k < 3; ++k) T.t[k] = translation[k];
  T.s = scale;
  bool finite = std::isfinite(T.s);
  for (int k = 0; k < 9; ++k) finite = finite && std::isfinite(T.R[k]);
  for (int k = 0; k < 3; ++k) finite = finite && std::isfinite(T.t[k]);
  if (!finite) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "non-finite transformation");
  if (num_cameras == 0 && num_points == 0) {
    if (timings_ms) { timings_ms[0] = 0.0; timings_ms[1] = ms_since(t_call); }
    return 0;
  }
  int rc = ensure_device();
  if (rc) return rc;
  const size_t nc = (size_t)num_cameras, np = (size_t)num_points;
  DevBuf<double> d_cam, d_pt;
  DevBuf<uint8_t> d_cm, d_pm;
  if ((rc = d_cam.up(cameras, 6 * nc)) || (rc = d_pt.up(points, 4 * np)) ||
      (camera_estimated && nc && (rc = d_cm.up(camera_estimated, nc))) || (point_estimated && np && (rc = d_pm.up(point_estimated, np))))
    return rc;
  KernelClock clk;
  HIP_TRY(clk.start(timings_ms != nullptr));
  k_transform<<<grid_of(nc + np, kThreads), kThreads>>>(num_cameras, d_cam.p, d_cm.p, (long long)num_points, d_pt.p, d_pm.p, T);
  HIP_TRY(hipGetLastError());
  float kernel_ms = 0.f;
  HIP_TRY(clk.stop(&kernel_ms));
  if (nc) HIP_TRY(hipMemcpy(cameras, d_cam.p, sizeof(double) * 6 * nc, hipMemcpyDeviceToHost));
  if (np) HIP_TRY(hipMemcpy(points, d_pt.p, sizeof(double) * 4 * np, hipMemcpyDeviceToHost));
  if (timings_ms) { timings_ms[0] = kernel_ms; timings_ms[1] = ms_since(t_call); }
  return 0;
}

extern "C" int theia_hip_align_rotations(int32_t num_rotations, const double* gt_rotation, double* rotation, double* alignment,
                                         theia_align_rotations_summary* summary, double* trace_out, int32_t trace_capacity) {
  const auto t_call = std::chrono::steady_clock::now();
  if (summary) *summary = theia_align_rotations_summary{};
  if (num_rotations < 1) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "at least one rotation is needed");
  if (!gt_rotation || !rotation || !alignment) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null array");
  if (trace_capacity < 0 || (trace_capacity > 0 && !trace_out)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "bad trace buffer");
  const size_t n = (size_t)num_rotations;
  for (size_t k = 0; k < 3 * n; ++k)
    if (!std::isfinite(gt_rotation[k]) || !std::isfinite(rotation[k]))
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "non-finite rotation %zu", k / 3);
  int rc = ensure_device();
  if (rc) return rc;
  DevBuf<double> d_gt, d_rot, d_Ru, d_trace;
  DevBuf<AlignRotState> d_state;
  const int rows_cap = trace_out ? trace_capacity : 0;
  if ((rc = d_gt.up(gt_rotation, 3 * n)) || (rc = d_rot.up(rotation, 3 * n)) || (rc = d_Ru.alloc(9 * n)) ||
      (rc = d_trace.alloc(5 * (size_t)rows_cap)) || (rc = d_state.alloc(1)))
    return rc;
  k_align_rotations<<<1, kThreads>>>(num_rotations, d_gt.p, d_rot.p, d_Ru.p, rows_cap ? d_trace.p : nullptr, rows_cap, d_state.p);
  HIP_TRY(hipGetLastError());
  AlignRotState h{};
  HIP_TRY(hipMemcpy(&h, d_state.p, sizeof(h), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(rotation, d_rot.p, sizeof(double) * 3 * n, hipMemcpyDeviceToHost));
  const int rows = std::min(h.trace_rows, rows_cap);
  if (rows > 0) HIP_TRY(hipMemcpy(trace_out, d_trace.p, sizeof(double) * 5 * (size_t)rows, hipMemcpyDeviceToHost));
  for (int k = 0; k < 3; ++k) alignment[k] = h.w[k];
  if (summary) {
    summary->iterations = h.iterations; summary->num_successful_steps = h.successful;
    summary->num_unsuccessful_steps = h.unsuccessful; summary->num_invalid_steps = h.invalid;
    summary->termination = h.term; summary->trace_size = rows;
    summary->initial_cost = h.initial_cost; summary->final_cost = h.cost; summary->final_radius = h.radius;
    summary->final_gradient_max_norm = h.gmax; summary->seconds = ms_since(t_call) * 1e-3;
  }
  return 0;
}
