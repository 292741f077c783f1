// ransac.hip -- many-hypothesis RANSAC on gfx950: K5 (minimal-solver fit) and
// K6 (score every correspondence under every model) plus the host driver (RansacCall, ransac_run) that
// replaces SampleConsensusEstimator<E>::Estimate
//   (src/theia/solvers/sample_consensus_estimator.h:300-415)
// for Ransac<E> + RandomSampler (ransac.h:57-61, random_sampler.cc:53-72).
//
// Split of work (DESIGN.md "RANSAC"):
//  host   : the std::mt19937 sample stream (bit-exact restatement, util/random.cc)
//           for a ROUND of iterations up front; sequential replay of the
//           accept / adaptive-termination rules in sample order (both in ransac_rng.h).
//  device : k_fit   -- one thread per hypothesis: minimal solver -> <= 10 models
//           k_score -- one thread per (hypothesis, model): walks all N
//                      correspondences (staged in LDS, broadcast reads) in data
//                      order, so the MLE sum keeps the reference's
//                      left-to-right FP64 order.
//  Hypotheses of a round are independent given the pre-generated samples, so a
//  batch of problems x iterations fills the chip; results are identical to the
//  sequential loop because acceptance is replayed in order.
// The streams entry point and theia_hip_rng_* are in ransac_streams.hip, the directly bound minimal solvers in
// ransac_solvers.hip (their kernels stay here, behind the launch_* functions of ransac_internal.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "ba_device.h"      // the camera models' projection (TriangulationEstimator::Error)
#include "ransac_device.h"
#include "dls_device.h"
#include "eig_team.h"
#include "fit5_team.h"
#include "svd_team.h"
#include "p4pf_device.h"
#include "alignment_device.h"   // CameraAlignmentEstimator
#include "theia_hip.h"
#include <atomic>
#include <mutex>
#include <thread>

#include "device_util.h"
#include "host_team.h"
#include "pools.h"
#include "ransac_internal.h"

namespace thip {
namespace {

constexpr int kMaxCap = 18;   // largest EstimateModel output of the thread-per-hypothesis solvers (SQPnP: 18 solutions)
constexpr int kMaxSampleDoubles = 6 * rsc::kRadHomDatum;   // 8 correspondences x 4, two observations with their cameras (66), six radial-distortion correspondences (72)
static_assert(kMaxSampleDoubles >= 2 * kTriDatum, "sample buffer");
// the sample buffer of a k_fit instance: 32 doubles for the correspondence estimators (their kernels keep the frame they had)
template <int EST> constexpr int sample_doubles() { return (EST == THEIA_EST_TRIANGULATION || EST == THEIA_EST_RADIAL_HOMOGRAPHY || EST < 0) ? kMaxSampleDoubles : 32; }

// EstimateModel of the three estimators (estimate_relative_pose.cc:75-109,
// estimate_essential_matrix.cc:62-73, estimate_calibrated_absolute_pose.cc:76-118).
// EST >= 0: compile-time estimator (k_fit: each instantiation carries only its own solver's scratch frame);
// EST < 0: runtime dispatch on `est`.
// estimator constants that are not data (UncalibratedRelativePoseEstimator's min / max focal length)
struct EstParams { double min_focal, max_focal; };

template <int EST = -1>
__device__ int estimate_models(int est, const double* subset, double* models, EstParams ep = EstParams{0.0, 0.0}) {
  if (EST >= 0) est = EST;
  constexpr bool any = EST < 0;
  if ((any || EST == THEIA_EST_RELATIVE_POSE || EST == THEIA_EST_ESSENTIAL_MATRIX) &&
      (est == THEIA_EST_RELATIVE_POSE || est == THEIA_EST_ESSENTIAL_MATRIX)) {
    double E[90];
    const int ne = rsc::five_point(subset, E);
    if (ne == 0) return 0;
    int nm = 0;
    for (int i = 0; i < ne; ++i) {
      double* m = models + kStride * nm;
      for (int k = 0; k < 9; ++k) m[k] = E[9 * i + k];
      if (est == THEIA_EST_ESSENTIAL_MATRIX) { for (int k = 9; k < kStride; ++k) m[k] = 0.0; nm++; continue; }
      const int nfront = rsc::best_pose_from_E(E + 9 * i, subset, 5, m + 9, m + 18);
      if (nfront >= 4) nm++;
    }
    return nm;
  }
  if ((any || EST == THEIA_EST_ABSOLUTE_POSE_KNEIP) && est == THEIA_EST_ABSOLUTE_POSE_KNEIP) {
    double Rs[36], ts[12];
    const int n = rsc::p3p(subset, Rs, ts);
    for (int i = 0; i < n; ++i) {
      double* m = models + kStride * i;
      const double* R = Rs + 9 * i;
      const double* t = ts + 3 * i;
      for (int k = 0; k < 9; ++k) m[k] = R[k];
      for (int c = 0; c < 3; ++c) m[9 + c] = -((R[c] * t[0] + R[3 + c] * t[1]) + R[6 + c] * t[2]);
      for (int k = 12; k < kStride; ++k) m[k] = 0.0;
    }
    return n;
  }
  if ((any || EST == THEIA_EST_ABSOLUTE_POSE_SQPNP) && est == THEIA_EST_ABSOLUTE_POSE_SQPNP) {
    // SQPnP on the 3 sampled correspondences; quaternion -> matrix as the estimator does
    // (estimate_calibrated_absolute_pose.cc:99-106)
    double feat[6], world[9], quats[72], ts[54];
    for (int i = 0; i < 3; ++i) {
      feat[2 * i] = subset[5 * i]; feat[2 * i + 1] = subset[5 * i + 1];
      for (int k = 0; k < 3; ++k) world[3 * i + k] = subset[5 * i + 2 + k];
    }
    const int n = rsc::sqpnp(3, feat, world, quats, ts);
    for (int i = 0; i < n; ++i) {
      double* m = models + kStride * i;
      double R[9];
      rsc::quat_to_rot(quats + 4 * i, R);
      const double* t = ts + 3 * i;
      for (int k = 0; k < 9; ++k) m[k] = R[k];
      for (int c = 0; c < 3; ++c) m[9 + c] = -((R[c] * t[0] + R[3 + c] * t[1]) + R[6 + c] * t[2]);
      for (int k = 12; k < kStride; ++k) m[k] = 0.0;
    }
    return n;
  }
  if ((any || EST == THEIA_EST_RADIAL_HOMOGRAPHY) && est == THEIA_EST_RADIAL_HOMOGRAPHY)   // estimate_radial_distortion_homography.cc:62-77
    return rsc::radial_homography_six_point(subset, models, kStride);
  // single-model estimators (estimate_fundamental_matrix.cc:64-78, estimate_homography.cc:72-88,
  // estimate_dominant_plane_from_points.cc:62-81, estimate_relative_pose_with_known_orientation.cc:31-45)
  if ((any || EST >= THEIA_EST_FUNDAMENTAL_MATRIX) && est >= THEIA_EST_FUNDAMENTAL_MATRIX) {
    bool ok = false;
    for (int k = 0; k < kStride; ++k) models[k] = 0.0;
    if (est == THEIA_EST_UNCALIBRATED_RELATIVE_POSE) {
      const double mm[2] = {ep.min_focal, ep.max_focal};
      ok = rsc::uncalibrated_relative_pose(subset, mm, models);
    }
    else if (est == THEIA_EST_ABSOLUTE_POSE_KNOWN_ORIENTATION) ok = rsc::position_from_two_rays(subset, models);
    else if (est == THEIA_EST_TRIANGULATION) ok = rsc::triangulate_two_views(subset, models);
    else if (est == THEIA_EST_FUNDAMENTAL_MATRIX) ok = rsc::eight_point_fundamental(subset, models);
    else if (est == THEIA_EST_HOMOGRAPHY) ok = rsc::four_point_homography(subset, models);
    else if (est == THEIA_EST_DOMINANT_PLANE) ok = rsc::plane_from_three_points(subset, models);
    else if (est == THEIA_EST_RELATIVE_POSE_KNOWN_ORIENTATION) ok = rsc::two_point_relative_position(subset, models);
    else if (est == THEIA_EST_CAMERA_ALIGNMENT) { rsc::camera_alignment_fit(subset, models); ok = true; }   // align_reconstructions.cc:66-84: always true
    return ok ? 1 : 0;
  }
  return 0;
}

// TriangulationEstimator::Error (estimate_triangulation.cc:92-101): Camera::ProjectPoint (camera.cc:206-216) of the
// homogeneous point -- adjusted = X.head<3>() - X[3] c, rotated by the angle-axis, pixel through the camera model (the
// BA kernels' projection, ba_device.h), depth = rotated.z / X[3] -- then the squared pixel error, DBL_MAX behind the camera.
__device__ inline double triangulation_error(const double* X, const double* d) {
  const double* ext = d + 16;
  const double p[3] = {X[0] - X[3] * ext[0], X[1] - X[3] * ext[1], X[2] - X[3] * ext[2]};
  RotTerms rt;
  rotation_terms(ext + 3, rt);
  const double q[3] = {(rt.R[0] * p[0] + rt.R[1] * p[1]) + rt.R[2] * p[2], (rt.R[3] * p[0] + rt.R[4] * p[1]) + rt.R[5] * p[2],
                       (rt.R[6] * p[0] + rt.R[7] * p[1]) + rt.R[8] * p[2]};
  const double depth = q[2] / X[3];
  if (depth <= 0.0) return DBL_MAX;
  double uv[2], Jq[6];
  project<false>((int)d[22], d + 23, q, uv, Jq);
  const double ex = d[14] - uv[0], ey = d[15] - uv[1];
  return ex * ex + ey * ey;
}

// Estimator::Error (estimate_relative_pose.cc:142-151, estimate_essential_matrix.cc:77-83,
// estimate_calibrated_absolute_pose.cc:158-167)
// GdlsSimilarityTransformationEstimator::Error (estimate_similarity_transformation_2d_3d.cc:137-155) with TransformCamera
// (:52-70): new position = s R c + t, new orientation = R_cam R^T, then Camera::ProjectPoint; DBL_MAX at negative depth.
__device__ inline double similarity_error(const double* m, const double* d) {
  const double* X = d + 3; const double* c = d + 9;
  double np[3], a[3], b[3];
  for (int r = 0; r < 3; ++r) np[r] = m[12] * ((m[3 * r] * c[0] + m[3 * r + 1] * c[1]) + m[3 * r + 2] * c[2]) + m[9 + r];
  for (int r = 0; r < 3; ++r) a[r] = X[r] - X[3] * np[r];
  for (int r = 0; r < 3; ++r) b[r] = (m[r] * a[0] + m[3 + r] * a[1]) + m[6 + r] * a[2];   // R^T a
  RotTerms rt;
  rotation_terms(d + 12, rt);
  const double q[3] = {(rt.R[0] * b[0] + rt.R[1] * b[1]) + rt.R[2] * b[2], (rt.R[3] * b[0] + rt.R[4] * b[1]) + rt.R[5] * b[2],
                       (rt.R[6] * b[0] + rt.R[7] * b[1]) + rt.R[8] * b[2]};
  if (q[2] / X[3] < 0.0) return DBL_MAX;
  double uv[2], Jq[6];
  project<false>((int)d[15], d + 16, q, uv, Jq);
  const double ex = d[7] - uv[0], ey = d[8] - uv[1];
  return ex * ex + ey * ey;
}

// NonCentralCameraPoseEstimator::Error (estimate_rigid_transformation_2d_3d.cc:116-129): R X + t through the datum's camera
// (Camera::ProjectPoint), DBL_MAX at negative depth.
__device__ inline double rigid_error(const double* m, const double* d) {
  const double* X = d + 3; const double* c = d + 9;
  const double h[3] = {X[0] / X[3], X[1] / X[3], X[2] / X[3]};
  double a[3];
  for (int r = 0; r < 3; ++r) a[r] = (((m[3 * r] * h[0] + m[3 * r + 1] * h[1]) + m[3 * r + 2] * h[2]) + m[9 + r]) - 1.0 * c[r];
  RotTerms rt;
  rotation_terms(d + 12, rt);
  const double q[3] = {(rt.R[0] * a[0] + rt.R[1] * a[1]) + rt.R[2] * a[2], (rt.R[3] * a[0] + rt.R[4] * a[1]) + rt.R[5] * a[2],
                       (rt.R[6] * a[0] + rt.R[7] * a[1]) + rt.R[8] * a[2]};
  if (q[2] / 1.0 < 0.0) return DBL_MAX;
  double uv[2], Jq[6];
  project<false>((int)d[15], d + 16, q, uv, Jq);
  const double ex = d[7] - uv[0], ey = d[8] - uv[1];
  return ex * ex + ey * ey;
}

// RadialDistUncalibratedAbsolutePoseEstimator::Error (estimate_radial_dist_uncalibrated_absolute_pose.cc:130-147) with DistortPoint
// (:56-74): the projection with the model's focal length, distorted by the division model, against the feature; 1e10 when the
// translation's z is negative.  m: rotation (9) | translation (3) | focal length | distortion; d: [u v X Y Z]
__device__ inline double radial_dist_error(const double* m, const double* d) {
  if (m[11] < 0.0) return 1.0e10;
  double p[3];
  for (int r = 0; r < 3; ++r) p[r] = ((m[3 * r] * d[2] + m[3 * r + 1] * d[3]) + m[3 * r + 2] * d[4]) + m[9 + r];
  const double kp[3] = {m[12] * p[0], m[12] * p[1], 1.0 * p[2]};
  const double x = kp[0] / kp[2], y = kp[1] / kp[2];
  const double r2 = x * x + y * y;
  const double denom = 2.0 * m[13] * r2, inner = 1.0 - 4.0 * m[13] * r2;
  double dx = x, dy = y;
  if (!(fabs(denom) < 1e-15 || inner < 0.0)) {
    const double sc = (1.0 - sqrt(inner)) / denom;
    dx = x * sc; dy = y * sc;
  }
  const double ex = dx - d[0], ey = dy - d[1];
  return ex * ex + ey * ey;
}

__device__ inline double model_error(int est, const double* m, const double* d) {
  if (est == THEIA_EST_RADIAL_DIST_UNCALIBRATED_ABSOLUTE_POSE) return radial_dist_error(m, d);
  if (est == THEIA_EST_UNCALIBRATED_ABSOLUTE_POSE) return p4pfdev::reprojection_error(m, d);
  if (est == THEIA_EST_SIMILARITY_2D3D) return similarity_error(m, d);
  if (est == THEIA_EST_RIGID_TRANSFORMATION_2D3D) return rigid_error(m, d);
  if (est == THEIA_EST_TRIANGULATION) return triangulation_error(m, d);
  if (est == THEIA_EST_RADIAL_HOMOGRAPHY) return rsc::radial_homography_error(m, d);
  if (est == THEIA_EST_RELATIVE_POSE) {
    if (rsc::in_front(d, m + 9, m + 18)) return rsc::sampson(m, d);
    return DBL_MAX;
  }
  if (est == THEIA_EST_ESSENTIAL_MATRIX || est == THEIA_EST_FUNDAMENTAL_MATRIX) return rsc::sampson(m, d);
  if (est == THEIA_EST_HOMOGRAPHY) return rsc::homography_error(m, d);
  if (est == THEIA_EST_DOMINANT_PLANE) return rsc::plane_error(m, d);
  if (est == THEIA_EST_RELATIVE_POSE_KNOWN_ORIENTATION) return rsc::known_orientation_error(m, d);
  if (est == THEIA_EST_UNCALIBRATED_RELATIVE_POSE) return rsc::uncalibrated_relative_pose_error(m, d);
  if (est == THEIA_EST_ABSOLUTE_POSE_KNOWN_ORIENTATION) return rsc::known_orientation_abs_error(m, d);
  if (est == THEIA_EST_CAMERA_ALIGNMENT) return rsc::camera_alignment_error(m, d);
  const double dx = d[2] - m[9], dy = d[3] - m[10], dz = d[4] - m[11];
  const double px = (m[0] * dx + m[1] * dy) + m[2] * dz;
  const double py = (m[3] * dx + m[4] * dy) + m[5] * dz;
  const double pz = (m[6] * dx + m[7] * dy) + m[8] * dz;
  const double ex = px / pz - d[0], ey = py / pz - d[1];
  return ex * ex + ey * ey;
}

// K5: one thread per (problem, iteration of the round).
//   samples : [nprob][B][m] indices into the problem's data
//   models  : [nprob][B][mm][kStride], mm = max_models(est)
//   counts  : [nprob][B]
template <int EST>
__global__ __launch_bounds__(64) void k_fit(int est, int nprob, int B, const int64_t* __restrict__ offsets,
                                            const double* __restrict__ data, const int* __restrict__ samples,
                                            const int* __restrict__ active_iters, double* __restrict__ models,
                                            int* __restrict__ counts, int* __restrict__ dense_count,
                                            int* __restrict__ tags, int* __restrict__ hyp_base, EstParams ep) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  const int p = blockIdx.y;
  if (b >= B || p >= nprob) return;
  const size_t hyp = (size_t)p * B + b;
  const int mm = max_models(est);
  if (b >= active_iters[p]) { counts[hyp] = 0; return; }
  const int m = sample_size(est), ds = datum_size(est);
  const double* pd = data + (size_t)offsets[p] * ds;
  double subset[sample_doubles<EST>()];
  for (int i = 0; i < m; ++i) {
    const int idx = samples[hyp * m + i];
    for (int k = 0; k < ds; ++k) subset[i * ds + k] = pd[(size_t)idx * ds + k];
  }
  double mloc[kMaxCap * kStride];
  const int nm = estimate_models<EST>(est, subset, mloc, ep);
  counts[hyp] = nm;
  if (nm == 0) return;
  // append to the problem's DENSE model list (most of the 10 slots per hypothesis
  // are empty: scoring a dense list keeps every lane of k_score busy); the tag
  // remembers (iteration, slot) so the host replays in sample order.
  const int base = atomicAdd(&dense_count[p], nm);
  hyp_base[hyp] = base;   // where this hypothesis' models start in the dense list (LO events fetch their model from there)
  double* mo = models + ((size_t)p * B * mm + base) * (size_t)kStride;
  int* tg = tags + (size_t)p * B * mm + base;
  for (int j = 0; j < nm; ++j) {
    for (int k = 0; k < kStride; ++k) mo[j * kStride + k] = mloc[j * kStride + k];
    tg[j] = b * mm + j;
  }
}

// K6: one thread per (problem, iteration, model slot); block = 256 slots of ONE
// problem, whose correspondences are staged in LDS when they fit.
// EST >= 0: the estimator is a compile-time constant (the error functions of the others drop out: the run-time dispatch
// keeps all of them -- the eight camera models of the triangulation error included -- in one 192-VGPR kernel at two waves
// per SIMD); EST < 0: run-time dispatch on `est`.
// The specialised instances run 512 slots per workgroup: the LDS copy of a problem's correspondences (64 - 80 KB at
// 2000 per pair) allows two workgroups per CU, i.e. four waves per SIMD instead of two.
constexpr int score_threads(int est) { return est >= 0 ? 512 : 256; }
template <bool USE_LDS, int EST = -1>
__global__ __launch_bounds__(score_threads(EST)) void k_score(int est_rt, int nprob, int B, const int64_t* __restrict__ offsets,
                                               const double* __restrict__ data, const double* __restrict__ models,
                                               const int* __restrict__ dense_count, const int* __restrict__ tags,
                                               double thresh, int use_mle, double* __restrict__ cost,
                                               int* __restrict__ ninl) {
  extern __shared__ __attribute__((aligned(16))) double sdata[];
  const int est = EST >= 0 ? EST : est_rt;
  const int p = blockIdx.y;
  const int nmodels = dense_count[p];
  if ((int)(blockIdx.x * blockDim.x) >= nmodels) return;  // whole block beyond the dense list
  const int ds = datum_size(est);
  const int64_t n64 = offsets[p + 1] - offsets[p];
  const int n = (int)n64;
  const double* pd = data + (size_t)offsets[p] * ds;
  if (USE_LDS) {
    for (int i = threadIdx.x; i < n * ds; i += blockDim.x) sdata[i] = pd[i];
    __syncthreads();
    pd = sdata;
  }
  const int slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= nmodels) return;
  const int mm = max_models(est);
  const size_t dense = (size_t)p * B * mm + slot;
  const size_t out = dense;   // scores stay in the dense order of the models (hyp_base[hyp] + slot): the host downloads them packed
  double m[kStride];
  const double* mo = models + dense * (size_t)kStride;
#pragma unroll
  for (int k = 0; k < kStride; ++k) m[k] = mo[k];
  int cnt = 0;
  double mle = 0.0;
  if (EST == THEIA_EST_RELATIVE_POSE || EST == THEIA_EST_ESSENTIAL_MATRIX) {
    // Sampson error without its division wherever the comparison is decided by the margin (twoview_device.h quotient_below)
    for (int i = 0; i < n; ++i) {
      const double* d = pd + (size_t)i * ds;
      bool in = false;
      double r = 0.0;
      if (EST == THEIA_EST_ESSENTIAL_MATRIX || rsc::in_front(d, m + 9, m + 18)) {
        double a, den;
        rsc::sampson_parts(m, d, &a, &den);
        in = rsc::quotient_below(a, den, thresh, use_mle != 0, &r);
      }
      if (in) { cnt++; mle += r; }
      else mle += thresh;
    }
  } else if (EST == THEIA_EST_ABSOLUTE_POSE_KNEIP || EST == THEIA_EST_ABSOLUTE_POSE_DLS || EST == THEIA_EST_ABSOLUTE_POSE_SQPNP) {
    // | hnormalized(R (X - c)) - x |^2 < thresh  (estimate_calibrated_absolute_pose.cc:158-167) decided WITHOUT its two divisions
    // wherever the margin allows: 1 / z from v_rcp_f64 + one Newton step (relative error < 2^-48: scripts/ubench/rcp_acc), the
    // error of the squared distance computed with it bounded by  r 2^-20 + (|x / z| + |y / z|)^2 2^-60  (a cancellation in
    // x / z - u costs absolute, not relative accuracy); inside that band -- and for an inlier whose value the MLE score adds --
    // the reference's arithmetic runs.  Same decisions, same sums: the two divisions were ~half of this loop's instructions.
    for (int i = 0; i < n; ++i) {
      const double* d = pd + (size_t)i * ds;
      const double dx = d[2] - m[9], dy = d[3] - m[10], dz = d[4] - m[11];
      const double px = (m[0] * dx + m[1] * dy) + m[2] * dz;
      const double py = (m[3] * dx + m[4] * dy) + m[5] * dz;
      const double pz = (m[6] * dx + m[7] * dy) + m[8] * dz;
      double iz = __builtin_amdgcn_rcp(pz);
      iz = __builtin_fma(iz, __builtin_fma(-pz, iz, 1.0), iz);
      const double qx = px * iz, qy = py * iz;
      const double ax = qx - d[0], ay = qy - d[1];
      const double ra = ax * ax + ay * ay;
      const double qq = fabs(qx) + fabs(qy);
      const double bound = ra * 0x1p-20 + (qq * qq) * 0x1p-60;
      if (ra - bound > thresh) { mle += thresh; continue; }          // surely an outlier (an outlier's value is never used)
      if (!use_mle && ra + bound < thresh) { cnt++; continue; }      // surely an inlier, and nobody asks for the value
      const double ex = px / pz - d[0], ey = py / pz - d[1];
      const double r = ex * ex + ey * ey;
      if (r < thresh) { cnt++; mle += r; }
      else mle += thresh;
    }
  } else {
    for (int i = 0; i < n; ++i) {
      const double r = model_error(est, m, pd + (size_t)i * ds);
      if (r < thresh) { cnt++; mle += r; }
      else mle += thresh;
    }
  }
  cost[out] = use_mle ? mle : (double)(n - cnt);
  ninl[out] = cnt;
}

// ---- LMED (lmed.h:64-70, lmed_quality_measurement.h:58-130): cost = median of the squared residuals, inliers by the
// 2.5 * 1.4826 * (1 + 5 / (n - m)) * sqrt(median) rule.  One workgroup per model: squared residuals in LDS, the order
// statistics by an 8-bit radix select on the IEEE bit patterns (exact: the median is an element, or the mean of two).
// sq == nullptr (more data than the LDS holds: > 19 456 per problem): the squared residuals are re-evaluated in every pass --
// the same bits each time, ten evaluations per datum instead of one; lmed_quality_measurement.h:56-63 has no size limit.
__device__ __forceinline__ double lmed_sq(const double* sq, int est, const double* m, const double* pd, int ds, int i) {
  if (sq) return sq[i];
  const double r = model_error(est, m, pd + (size_t)i * ds);
  return r * r;
}
__device__ double lmed_select(const double* sq, int n, int k, int* hist, int* sel, int est, const double* m, const double* pd, int ds) {
  unsigned long long prefix = 0ull, mask = 0ull;
  for (int shift = 56; shift >= 0; shift -= 8) {
    for (int b = threadIdx.x; b < 256; b += blockDim.x) hist[b] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      const unsigned long long key = (unsigned long long)__double_as_longlong(lmed_sq(sq, est, m, pd, ds, i));
      if ((key & mask) == prefix) atomicAdd(&hist[(int)((key >> shift) & 255ull)], 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int cum = 0, b = 0;
      for (; b < 255; ++b) { if (cum + hist[b] > k) break; cum += hist[b]; }
      sel[0] = b; sel[1] = k - cum;
    }
    __syncthreads();
    prefix |= (unsigned long long)sel[0] << shift;
    mask |= 255ull << shift;
    k = sel[1];
    __syncthreads();
  }
  return __longlong_as_double((long long)prefix);
}

// returns the median (cost); *ninl = inlier count; mask (optional, global) receives the inlier flags
__device__ double lmed_block(int est, const double* m, const double* pd, int n, int ds, int min_samples, double* sq,
                             int* hist, int* sel, int* ninl, uint8_t* mask, double* sqt_out = nullptr) {
  if (sq) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) { const double r = model_error(est, m, pd + (size_t)i * ds); sq[i] = r * r; }
  }
  __syncthreads();
  double median = lmed_select(sq, n, n / 2, hist, sel, est, m, pd, ds);
  if ((n % 2) != 0) median = 0.5 * (lmed_select(sq, n, n / 2 - 1, hist, sel, est, m, pd, ds) + median);
  const double thr = 2.5 * 1.4826 * (1 + 5.0 / (double)((size_t)n - (size_t)min_samples)) * sqrt(median);
  const double sqt = thr * thr;
  if (sqt_out && threadIdx.x == 0) *sqt_out = sqt;
  if (threadIdx.x == 0) sel[2] = 0;
  __syncthreads();
  int cnt = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const bool in = lmed_sq(sq, est, m, pd, ds, i) < sqt;
    cnt += in ? 1 : 0;
    if (mask) mask[i] = in ? 1 : 0;
  }
  atomicAdd(&sel[2], cnt);
  __syncthreads();
  *ninl = sel[2];
  return median;
}

__global__ __launch_bounds__(256) void k_score_lmed(int est, int nprob, int B, const int64_t* __restrict__ offsets,
                                                    const double* __restrict__ data, const double* __restrict__ models,
                                                    const int* __restrict__ dense_count, const int* __restrict__ tags,
                                                    double* __restrict__ cost, int* __restrict__ ninl, int in_lds) {
  extern __shared__ __attribute__((aligned(16))) double sdata[];
  __shared__ int hist[256], sel[4];
  __shared__ double m[kStride];
  const int p = blockIdx.y, slot = blockIdx.x;
  if (slot >= dense_count[p]) return;
  const int mm = max_models(est), ds = datum_size(est);
  const int n = (int)(offsets[p + 1] - offsets[p]);
  const size_t dense = (size_t)p * B * mm + slot;
  if (threadIdx.x < kStride) m[threadIdx.x] = models[dense * (size_t)kStride + threadIdx.x];
  __syncthreads();
  int cnt;
  const double med = lmed_block(est, m, data + (size_t)offsets[p] * ds, n, ds, sample_size(est), in_lds ? sdata : nullptr, hist, sel, &cnt, nullptr);
  if (threadIdx.x == 0) {
    const size_t out = dense;
    cost[out] = med; ninl[out] = cnt;
  }
}

__global__ __launch_bounds__(256) void k_inlier_mask_lmed(int est, int nprob, const int64_t* __restrict__ offsets,
                                                          const double* __restrict__ data, const double* __restrict__ best_models,
                                                          uint8_t* __restrict__ mask, int in_lds) {
  extern __shared__ __attribute__((aligned(16))) double sdata[];
  __shared__ int hist[256], sel[4];
  __shared__ double m[kStride];
  const int p = blockIdx.x;
  const int ds = datum_size(est);
  const int n = (int)(offsets[p + 1] - offsets[p]);
  if (threadIdx.x < kStride) m[threadIdx.x] = best_models[(size_t)p * kStride + threadIdx.x];
  __syncthreads();
  int cnt;
  lmed_block(est, m, data + (size_t)offsets[p] * ds, n, ds, sample_size(est), in_lds ? sdata : nullptr, hist, sel, &cnt, mask + offsets[p]);
}

// LO under LMED: the inliers RefineModel sees are the quality measurement's own (r^2 < its median-derived bound): the bound of
// every LO event's model, for k_lo_gather
__global__ __launch_bounds__(256) void k_lo_lmed_bound(int est, const int* __restrict__ ev_prob, const int64_t* __restrict__ offsets,
                                                       const double* __restrict__ data, const double* __restrict__ ev_model,
                                                       double* __restrict__ ev_sqt, int in_lds) {
  extern __shared__ __attribute__((aligned(16))) double sdata[];
  __shared__ int hist[256], sel[4];
  __shared__ double m[kStride];
  const int e = blockIdx.x, p = ev_prob[e];
  const int ds = datum_size(est);
  const int n = (int)(offsets[p + 1] - offsets[p]);
  if (threadIdx.x < kStride) m[threadIdx.x] = ev_model[(size_t)e * kStride + threadIdx.x];
  __syncthreads();
  int cnt;
  lmed_block(est, m, data + (size_t)offsets[p] * ds, n, ds, sample_size(est), in_lds ? sdata : nullptr, hist, sel, &cnt, nullptr, ev_sqt + e);
}

// final pass: refit the winning hypothesis (deterministic -> identical model)
// and mark the inliers of every datum (sample_consensus_estimator.h:396-399).
__global__ void k_refit(int est, int nprob, const int64_t* __restrict__ offsets, const double* __restrict__ data,
                        const int* __restrict__ best_samples, const int* __restrict__ best_slot,
                        double* __restrict__ out_models, EstParams ep) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nprob) return;
  double* mo = out_models + (size_t)p * kStride;
  for (int k = 0; k < kStride; ++k) mo[k] = 0.0;
  if (best_slot[p] < 0) return;
  const int m = sample_size(est), ds = datum_size(est);
  const double* pd = data + (size_t)offsets[p] * ds;
  double subset[kMaxSampleDoubles];
  for (int i = 0; i < m; ++i) {
    const int idx = best_samples[p * kMaxSample + i];
    for (int k = 0; k < ds; ++k) subset[i * ds + k] = pd[(size_t)idx * ds + k];
  }
  double mloc[kMaxCap * kStride];
  const int nm = estimate_models(est, subset, mloc, ep);
  const int j = best_slot[p];
  if (j < nm) for (int k = 0; k < kStride; ++k) mo[k] = mloc[j * kStride + k];
}

// after a round's replay: the problems whose best model changed in this round copy it out of the round's dense model
// list (the final models then need no refit: a single-thread five-point solve is ~2 ms of latency)
__global__ void k_save_best(int est, int n, const int* __restrict__ prob, const int* __restrict__ hyp, const int* __restrict__ slot,
                            int round_B, const double* __restrict__ round_models, const int* __restrict__ hyp_base,
                            double* __restrict__ best_models) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * kStride) return;
  const int e = i / kStride, k = i % kStride;
  const int h = hyp[e], q = h / round_B;
  best_models[(size_t)prob[e] * kStride + k] =
      round_models[((size_t)q * round_B * max_models(est) + hyp_base[h] + slot[e]) * (size_t)kStride + k];
}

// scores of a round, packed over the problems of the chunk for the download: problem q's dense_count[q] entries (stride
// B * mm on the device) go to [prefix[q], prefix[q + 1]).  The host reads model j of hypothesis h at prefix[q] + hyp_base[h] + j.
__global__ void k_pack_scores(int B, int mm, const int* __restrict__ dense_count, const int* __restrict__ prefix,
                              const double* __restrict__ cost, const int* __restrict__ ninl, double* __restrict__ pcost,
                              int* __restrict__ pninl) {
  const int q = blockIdx.y;
  const int n = dense_count[q];
  const size_t src = (size_t)q * B * mm;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    pcost[prefix[q] + i] = cost[src + i];
    pninl[prefix[q] + i] = ninl[src + i];
  }
}

__global__ void k_inlier_mask(int est, int nprob, const int64_t* __restrict__ offsets, const double* __restrict__ data,
                              const double* __restrict__ best_models, double thresh, uint8_t* __restrict__ mask) {
  const int p = blockIdx.y;
  const int ds = datum_size(est);
  const int n = (int)(offsets[p + 1] - offsets[p]);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double m[kStride];
  for (int k = 0; k < kStride; ++k) m[k] = best_models[(size_t)p * kStride + k];
  const double r = model_error(est, m, data + ((size_t)offsets[p] + i) * ds);
  mask[offsets[p] + i] = (r < thresh) ? 1 : 0;
}

// batched minimal solvers (directly bound entry points)
__global__ void k_five_point(int num, const double* __restrict__ corr, double* __restrict__ E, int* __restrict__ nsol) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num) return;
  double c[20], e[90];
  for (int k = 0; k < 20; ++k) c[k] = corr[(size_t)i * 20 + k];
  const int n = rsc::five_point(c, e);
  nsol[i] = n;
  for (int k = 0; k < 90; ++k) E[(size_t)i * 90 + k] = (k < 9 * n) ? e[k] : 0.0;
}

__global__ void k_p3p(int num, const double* __restrict__ corr, double* __restrict__ R, double* __restrict__ t, int* __restrict__ nsol) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num) return;
  double c[15], r[36], tt[12];
  for (int k = 0; k < 15; ++k) c[k] = corr[(size_t)i * 15 + k];
  const int n = rsc::p3p(c, r, tt);
  nsol[i] = n;
  for (int k = 0; k < 36; ++k) R[(size_t)i * 36 + k] = (k < 9 * n) ? r[k] : 0.0;
  for (int k = 0; k < 12; ++k) t[(size_t)i * 12 + k] = (k < 3 * n) ? tt[k] : 0.0;
}

// ---- LO-RANSAC refinement of the absolute-pose estimator (RefineModel,
// estimate_calibrated_absolute_pose.cc:120-153): the events of all problems of a
// replay round are refined as ONE batch of single-view LM solves (ba_batch.hip).
// An event = (problem, model source); source: refit from (samples, slot), or the
// problem's current best model.
__global__ void k_lo_prepare(int est, int nev, const int* __restrict__ ev_prob, const int* __restrict__ ev_samples,
                             const int* __restrict__ ev_slot, const int* __restrict__ ev_hyp, int round_B,
                             const double* __restrict__ round_models, const int* __restrict__ hyp_base,
                             const int64_t* __restrict__ offsets,
                             const double* __restrict__ data, const double* __restrict__ cur_models,
                             double* __restrict__ ev_model, double* __restrict__ ev_cam, EstParams ep) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nev) return;
  const int p = ev_prob[e];
  double mo[kStride];
  for (int k = 0; k < kStride; ++k) mo[k] = 0.0;
  if (ev_slot[e] < 0) {
    for (int k = 0; k < kStride; ++k) mo[k] = cur_models[(size_t)p * kStride + k];
  } else if (ev_hyp[e] >= 0) {
    // an event of the round being replayed: its model is still in the round's dense list (k_fit), the same bits a
    // refit would give -- a single-thread five-point refit costs ~2 ms of latency per LO batch
    const int h = ev_hyp[e];
    const int q = h / round_B;   // problem inside the chunk
    const double* src = round_models + ((size_t)q * round_B * max_models(est) + hyp_base[h] + ev_slot[e]) * (size_t)kStride;
    for (int k = 0; k < kStride; ++k) mo[k] = src[k];
  } else {
    const int m = sample_size(est), ds = datum_size(est);
    const double* pd = data + (size_t)offsets[p] * ds;
    double subset[kMaxSampleDoubles];
    for (int i = 0; i < m; ++i) {
      const int idx = ev_samples[e * kMaxSample + i];
      for (int k = 0; k < ds; ++k) subset[i * ds + k] = pd[(size_t)idx * ds + k];
    }
    double mloc[kMaxCap * kStride];
    const int nm = estimate_models(est, subset, mloc, ep);
    if (ev_slot[e] < nm) for (int k = 0; k < kStride; ++k) mo[k] = mloc[ev_slot[e] * kStride + k];
  }
  for (int k = 0; k < kStride; ++k) ev_model[(size_t)e * kStride + k] = mo[k];
  if (est == THEIA_EST_FUNDAMENTAL_MATRIX) {   // nine doubles per event, row-major
    double* fc = ev_cam + (size_t)e * 9;
    for (int k = 0; k < 9; ++k) fc[k] = mo[k];
    return;
  }
  if (est == THEIA_EST_HOMOGRAPHY) {   // homography->data(): Eigen's column-major storage order, nine doubles per event
    double* hc = ev_cam + (size_t)e * 9;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) hc[i + 3 * j] = mo[3 * i + j];
    return;
  }
  double* c = ev_cam + (size_t)e * 6;
  if (est == THEIA_EST_RELATIVE_POSE || est == THEIA_EST_UNCALIBRATED_RELATIVE_POSE) {
    // TwoViewInfo{rotation_2, position_2} of RefineModel (estimate_relative_pose.cc:115-118, estimate_uncalibrated_relative_pose.cc:157-160)
    rsc::eigen_rot_to_rotvec(mo + 9, c);
    c[3] = mo[18]; c[4] = mo[19]; c[5] = mo[20];
    return;
  }
  // Camera::SetPosition / SetOrientationFromRotationMatrix
  c[0] = mo[9]; c[1] = mo[10]; c[2] = mo[11];
  rsc::rot_to_angle_axis(mo, c + 3);
}

// inliers of the event's model, in data order, compacted as (uv, X, 1) for the view batch (absolute pose) or as
// correspondences for the two-view batch (relative pose); one wave per event
__global__ __launch_bounds__(64) void k_lo_gather(int est, const int* __restrict__ ev_prob, const int64_t* __restrict__ offsets,
                                                  const double* __restrict__ data, const double* __restrict__ ev_model,
                                                  double thresh, const double* __restrict__ ev_sqt /* LMED: per-event bound on r^2, else null */,
                                                  const int64_t* __restrict__ ev_off, int* __restrict__ ev_count,
                                                  double2* __restrict__ uv, double4* __restrict__ X) {
  const int e = blockIdx.x, lane = threadIdx.x;
  const int p = ev_prob[e];
  const int n = (int)(offsets[p + 1] - offsets[p]);
  const int ds = datum_size(est);
  const double* pd = data + (size_t)offsets[p] * ds;
  double m[kStride];
  for (int k = 0; k < kStride; ++k) m[k] = ev_model[(size_t)e * kStride + k];
  int base = 0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    bool in = false;
    if (i < n) {
      const double r = model_error(est, m, pd + (size_t)i * ds);
      in = ev_sqt ? (r * r < ev_sqt[e]) : (r < thresh);
    }
    const unsigned long long b = __ballot(in);
    if (in) {
      const int pos = base + __popcll(b & ((1ull << lane) - 1ull));
      const double* d = pd + (size_t)i * ds;
      if (est == THEIA_EST_RELATIVE_POSE || est == THEIA_EST_HOMOGRAPHY || est == THEIA_EST_FUNDAMENTAL_MATRIX) {   // the correspondence itself
        X[ev_off[e] + pos] = make_double4(d[0], d[1], d[2], d[3]);
      } else if (est == THEIA_EST_UNCALIBRATED_RELATIVE_POSE) {   // normalised by the model's focal lengths (:146-155)
        X[ev_off[e] + pos] = make_double4(d[0] / m[21], d[1] / m[21], d[2] / m[22], d[3] / m[22]);
      } else {
        uv[ev_off[e] + pos] = make_double2(d[0], d[1]);
        X[ev_off[e] + pos] = make_double4(d[2], d[3], d[4], 1.0);
      }
    }
    base += __popcll(b);
  }
  if (lane == 0) ev_count[e] = base;
}

// refined pose back into the problem's model (written even when RefineModel returns false)
__global__ void k_lo_finish(int est, int nev, const int* __restrict__ ev_prob, const double* __restrict__ ev_cam,
                            const double* __restrict__ ev_model, const BatchLmOut* __restrict__ out, double* __restrict__ cur_models,
                            int* __restrict__ ev_success) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nev) return;
  const int p = ev_prob[e];
  double* mo = cur_models + (size_t)p * kStride;
  if (est == THEIA_EST_FUNDAMENTAL_MATRIX) {   // estimate_fundamental_matrix.cc:82-90
    const double* fc = ev_cam + (size_t)e * 9;
    for (int k = 0; k < 9; ++k) mo[k] = fc[k];
    for (int k = 9; k < kStride; ++k) mo[k] = 0.0;
    ev_success[e] = (out[e].c1 < out[e].c0 && out[e].success) ? 1 : 0;
    return;
  }
  if (est == THEIA_EST_HOMOGRAPHY) {   // estimate_homography.cc:100-103: H (already divided by H(2,2)) replaces the model
    const double* hc = ev_cam + (size_t)e * 9;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) mo[3 * i + j] = hc[i + 3 * j];
    for (int k = 9; k < kStride; ++k) mo[k] = 0.0;
    ev_success[e] = (out[e].c1 < out[e].c0) ? 1 : 0;
    return;
  }
  const double* c = ev_cam + (size_t)e * 6;
  if (est == THEIA_EST_RELATIVE_POSE || est == THEIA_EST_UNCALIBRATED_RELATIVE_POSE) {
    // estimate_relative_pose.cc:130-135 / estimate_uncalibrated_relative_pose.cc:170-175: rotation and position are
    // replaced, the essential (fundamental) matrix and the focal lengths of the model are NOT recomputed -- Error keeps
    // scoring the Sampson distance of the unrefined matrix.  Success = the cost went down (and, uncalibrated, no FAILURE).
    for (int k = 0; k < kStride; ++k) mo[k] = ev_model[(size_t)e * kStride + k];
    rsc::eigen_rotvec_to_rot(c, mo + 9);
    mo[18] = c[3]; mo[19] = c[4]; mo[20] = c[5];
    const bool ok = out[e].c1 < out[e].c0;
    ev_success[e] = (est == THEIA_EST_RELATIVE_POSE ? ok : (ok && out[e].success)) ? 1 : 0;
    return;
  }
  rsc::angle_axis_to_rot(c + 3, mo);
  mo[9] = c[0]; mo[10] = c[1]; mo[11] = c[2];
  for (int k = 12; k < kStride; ++k) mo[k] = 0.0;
  ev_success[e] = (out[e].c1 < out[e].c0 && out[e].success) ? 1 : 0;
}

__global__ void k_select_models(int nprob, const int* __restrict__ use_cur, const double* __restrict__ cur_models,
                                double* __restrict__ best_models) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nprob || !use_cur[p]) return;
  for (int k = 0; k < kStride; ++k) best_models[(size_t)p * kStride + k] = cur_models[(size_t)p * kStride + k];
}

// SQPnP on problems of any size (the directly bound solver, sfm.cc:592): one thread per problem
__global__ void k_sqpnp(int num, const int64_t* __restrict__ offsets, const double* __restrict__ feat,
                        const double* __restrict__ world, double* __restrict__ quats, double* __restrict__ ts,
                        int* __restrict__ nsol) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num) return;
  double q[72], t[54];
  const int64_t o = offsets[i];
  const int n = rsc::sqpnp((int)(offsets[i + 1] - o), feat + 2 * o, world + 3 * o, q, t);
  nsol[i] = n;
  for (int k = 0; k < 72; ++k) quats[(size_t)i * 72 + k] = (k < 4 * n) ? q[k] : 0.0;
  for (int k = 0; k < 54; ++k) ts[(size_t)i * 54 + k] = (k < 3 * n) ? t[k] : 0.0;
}


// ---- five-point hypotheses (relative pose / essential matrix) in three stages instead of k_fit: the null space, the
// constraint matrix and its elimination (5 KB of work arrays per hypothesis) and the 10 x 10 eigen-decomposition (27 k
// read-modify-writes of its two work matrices) were per-lane scratch, i.e. HBM traffic (~200 KB per hypothesis for the
// eigen-solver alone); both run on chip now, by teams of lanes per hypothesis with the arrays in LDS (fit5_team.h,
// eig_team.h: bit-identical to the one-thread routines).  After them one thread per hypothesis turns the real
// eigenvectors into essential matrices and poses exactly as estimate_models() does.
constexpr int kFpWs = 136;    // per hypothesis: null space N (9 x 4) | action matrix M (10 x 10)

// stage A by teams of 16 lanes with the work arrays in LDS (fit5_team.h): N and M bit-identical to five_point_pre()
constexpr int kFpPreTeam = 16;
__global__ __launch_bounds__(64, 4) void k_fit5_a_team(int nprob, int B, const int64_t* __restrict__ offsets, const double* __restrict__ data,
                                                    const int* __restrict__ samples, const int* __restrict__ active_iters,
                                                    double* __restrict__ ws, int* __restrict__ ok) {
  __shared__ double lds[64 / kFpPreTeam][rsc::kFit5TeamLds];
  const int team = threadIdx.x / kFpPreTeam, tl = threadIdx.x % kFpPreTeam;
  const size_t hyp = (size_t)blockIdx.x * (64 / kFpPreTeam) + team;
  if (hyp >= (size_t)nprob * B) return;
  const int p = (int)(hyp / B), b = (int)(hyp % B);
  if (b >= active_iters[p]) { if (tl == 0) ok[hyp] = 0; return; }
  double* w = ws + hyp * kFpWs;
  const bool good = rsc::five_point_pre_team<kFpPreTeam>(data + (size_t)offsets[p] * 4, samples + hyp * 5, lds[team], w, w + 36, tl);
  if (tl == 0) ok[hyp] = good ? 1 : 0;
}

// stage B: teams of 8 lanes (eig_team.h), H and V in LDS, the work array X of the back-substitution in the hypothesis' own
// action-matrix slot in HBM (free once H is on chip).  The kernel is bound by the number of matrices resident per CU --
// the eigen-iteration is one dependent chain per matrix -- i.e. by LDS per matrix: 1.8 KB here (87 matrices per CU), and
// the same time with 16 or 8 lanes per team (measured), so the narrower team only halves the LDS per wave.
constexpr int kFpTeam = 8, kFpTeamsPerWave = 64 / kFpTeam;
template <bool P4PF = false>   // P4PF: the same eigen stage for the P4Pf action matrix; sol = rows 0..4 of the real eigenvectors
__global__ __launch_bounds__(64) void k_fit5_b(size_t nhyp, const int* __restrict__ ok, double* __restrict__ ws,
                                               double* __restrict__ sol, int* __restrict__ solmask) {
  __shared__ double lds[kFpTeamsPerWave][230];   // H (100) | V (100) | wr | wi | ort
  const int team = threadIdx.x / kFpTeam, tl = threadIdx.x % kFpTeam;
  const size_t hyp = (size_t)blockIdx.x * kFpTeamsPerWave + team;
  if (hyp >= nhyp) return;
  if (!ok[hyp]) { if (tl == 0) solmask[hyp] = 0; return; }
  double* H = lds[team]; double* V = H + 100; double* wr = V + 100; double* wi = wr + 10; double* ort = wi + 10;
  double* M = ws + hyp * kFpWs + 36;
  double* X = M;
  for (int e = tl; e < 100; e += kFpTeam) H[e] = M[e];
  rsc::team_sync();
  const bool good = rsc::eig_team<kFpTeam, false>(10, H, V, X, wr, wi, ort, tl);
  int bit = 0;
  for (int c = tl; c < 10; c += kFpTeam)
    if (good && wi[c] == 0.0) {   // only real solutions (five_point_relative_pose.cc:281-284)
      if (P4PF) {
        for (int k = 0; k < 5; ++k) sol[(hyp * 10 + c) * 5 + k] = V[k * 10 + c];
      } else {
        double v4[4];
        rsc::five_point_v4(V, c, v4);
        for (int k = 0; k < 4; ++k) sol[(hyp * 10 + c) * 4 + k] = v4[k];
      }
      bit |= 1 << c;
    }
  for (int o = kFpTeam / 2; o >= 1; o >>= 1) bit |= __shfl_xor(bit, o, kFpTeam);
  if (tl == 0) solmask[hyp] = bit;
}

// ---- SQPnP fit in three stages (sqpnp_pre -> 9 x 9 SVD by teams of nine lanes in LDS -> sqpnp_post): the SVD was 77 % of
// the one-thread-per-hypothesis kernel, whose 12.6 KB of arrays per lane lived in scratch.
// ws per hypothesis: [Omega 81 | P 27 | centroid 3 | U 81 | S 9]
#ifndef THIP_SQ_TEAM
#define THIP_SQ_TEAM 5   // lanes per 9 x 9 SVD (svd_team.h): 5 -> twelve matrices per wave; 9 (seven per wave) was rounds 3 - 5
#endif
constexpr int kSqWs = 201, kSqTeam = THIP_SQ_TEAM, kSqTeamsPerWave = 64 / kSqTeam;
__global__ __launch_bounds__(64) void k_sqp_a(int nprob, int B, const int64_t* __restrict__ offsets, const double* __restrict__ data,
                                              const int* __restrict__ samples, const int* __restrict__ active_iters,
                                              double* __restrict__ ws, int* __restrict__ ok) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  const int p = blockIdx.y;
  if (b >= B || p >= nprob) return;
  const size_t hyp = (size_t)p * B + b;
  if (b >= active_iters[p]) { ok[hyp] = 0; return; }
  const double* pd = data + (size_t)offsets[p] * 5;
  double feat[6], world[9];
  for (int i = 0; i < 3; ++i) {
    const int idx = samples[hyp * 3 + i];
    feat[2 * i] = pd[(size_t)idx * 5]; feat[2 * i + 1] = pd[(size_t)idx * 5 + 1];
    for (int k = 0; k < 3; ++k) world[3 * i + k] = pd[(size_t)idx * 5 + 2 + k];
  }
  double Om[81], P[27], mean[3];
  const bool good = rsc::sqpnp_pre(3, feat, world, Om, P, mean);
  ok[hyp] = good ? 1 : 0;
  if (!good) return;
  double* w = ws + hyp * kSqWs;
  for (int k = 0; k < 81; ++k) w[k] = Om[k];
  for (int k = 0; k < 27; ++k) w[81 + k] = P[k];
  for (int k = 0; k < 3; ++k) w[108 + k] = mean[k];
}

__global__ __launch_bounds__(64) void k_sqp_b(size_t nhyp, const int* __restrict__ ok, double* __restrict__ ws) {
  __shared__ double lds[kSqTeamsPerWave][81 + 81 + 9];   // W | U | S
  const int team = threadIdx.x / kSqTeam, tl = threadIdx.x % kSqTeam;
  if (team >= kSqTeamsPerWave) return;
  const size_t hyp = (size_t)blockIdx.x * kSqTeamsPerWave + team;
  if (hyp >= nhyp || !ok[hyp]) return;
  double* W = lds[team]; double* U = W + 81; double* S = U + 81;
  double* w = ws + hyp * kSqWs;
  rsc::svd9_team<kSqTeam>(w, W, U, S, tl);
  for (int e = tl; e < 9; e += kSqTeam) {
    for (int i = 0; i < 9; ++i) w[111 + i * 9 + e] = U[i * 9 + e];
    w[192 + e] = S[e];
  }
}

__global__ __launch_bounds__(64) void k_sqp_c(int nprob, int B, const int* __restrict__ active_iters, const int* __restrict__ ok,
                                              const double* __restrict__ ws, double* __restrict__ models, int* __restrict__ counts,
                                              int* __restrict__ dense_count, int* __restrict__ tags, int* __restrict__ hyp_base) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  const int p = blockIdx.y;
  if (b >= B || p >= nprob) return;
  const size_t hyp = (size_t)p * B + b;
  if (b >= active_iters[p] || !ok[hyp]) { counts[hyp] = 0; return; }
  const double* w = ws + hyp * kSqWs;
  double quats[72], ts[54];
  // Omega, P, the centroid, U and S are read where they lie (201 doubles of the workspace row): copies in per-lane arrays
  // would double the scratch frame of this kernel
  const int nm = rsc::sqpnp_post_impl(w, w + 81, w + 108, w + 111, w + 192, quats, ts);
  counts[hyp] = nm;
  if (nm == 0) return;
  constexpr int mm = 18;   // max_models(THEIA_EST_ABSOLUTE_POSE_SQPNP)
  const int base = atomicAdd(&dense_count[p], nm);
  hyp_base[hyp] = base;
  double* mo = models + ((size_t)p * B * mm + base) * (size_t)kStride;
  int* tg = tags + (size_t)p * B * mm + base;
  for (int j = 0; j < nm; ++j) {   // quaternion -> matrix as the estimator does (estimate_calibrated_absolute_pose.cc:99-106)
    double R[9];
    rsc::quat_to_rot(quats + 4 * j, R);
    const double* t = ts + 3 * j;
    double* m = mo + (size_t)j * kStride;
    for (int k = 0; k < 9; ++k) m[k] = R[k];
    for (int c = 0; c < 3; ++c) m[9 + c] = -((R[c] * t[0] + R[3 + c] * t[1]) + R[6 + c] * t[2]);
    for (int k = 12; k < kStride; ++k) m[k] = 0.0;
    tg[j] = b * mm + j;
  }
}

template <int EST>
__global__ __launch_bounds__(64) void k_fit5_c(int nprob, int B, const int64_t* __restrict__ offsets, const double* __restrict__ data,
                                               const int* __restrict__ samples, const int* __restrict__ active_iters,
                                               const double* __restrict__ ws, const double* __restrict__ sol,
                                               const int* __restrict__ solmask, double* __restrict__ models,
                                               int* __restrict__ counts, int* __restrict__ dense_count, int* __restrict__ tags,
                                               int* __restrict__ hyp_base) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  const int p = blockIdx.y;
  if (b >= B || p >= nprob) return;
  const size_t hyp = (size_t)p * B + b;
  if (b >= active_iters[p]) { counts[hyp] = 0; return; }
  const int mask = solmask[hyp];
  if (!mask) { counts[hyp] = 0; return; }
  const double* pd = data + (size_t)offsets[p] * 4;
  double subset[20];
  for (int i = 0; i < 5; ++i) {
    const int idx = samples[hyp * 5 + i];
    for (int k = 0; k < 4; ++k) subset[i * 4 + k] = pd[(size_t)idx * 4 + k];
  }
  double N[36];
  for (int k = 0; k < 36; ++k) N[k] = ws[hyp * kFpWs + k];
  double mloc[10 * kStride];
  int nm = 0;
  for (int i = 0; i < 10; ++i) {
    if (!((mask >> i) & 1)) continue;
    double v4[4];
    for (int k = 0; k < 4; ++k) v4[k] = sol[(hyp * 10 + i) * 4 + k];
    double* m = mloc + kStride * nm;
    rsc::five_point_E(N, v4, m);
    if (EST == THEIA_EST_ESSENTIAL_MATRIX) { for (int k = 9; k < kStride; ++k) m[k] = 0.0; nm++; continue; }
    const int nfront = rsc::best_pose_from_E(m, subset, 5, m + 9, m + 18);
    if (nfront >= 4) nm++;
  }
  counts[hyp] = nm;
  if (nm == 0) return;
  const int mm = 10;
  const int base = atomicAdd(&dense_count[p], nm);
  hyp_base[hyp] = base;
  double* mo = models + ((size_t)p * B * mm + base) * (size_t)kStride;
  int* tg = tags + (size_t)p * B * mm + base;
  for (int j = 0; j < nm; ++j) {
    for (int k = 0; k < kStride; ++k) mo[j * kStride + k] = mloc[j * kStride + k];
    tg[j] = b * mm + j;
  }
}

// ---- P4Pf hypotheses (uncalibrated absolute pose) in three stages (p4pf_device.h): the transposed elimination template by one
// workgroup per hypothesis in LDS -> the five-point kernel's 10 x 10 eigen stage -> one thread per hypothesis for the
// projection matrices.  ws per hypothesis: [normalisation 36 | action matrix 100] (the five-point layout: kFpWs).
static_assert(p4pfdev::kWs == kFpWs, "the P4Pf workspace row shares the five-point eigen stage");
__global__ __launch_bounds__(p4pfdev::kThreads) void k_p4pf_a(int nprob, int B, const int64_t* __restrict__ offsets, const double* __restrict__ data,
                                                            const int* __restrict__ samples, const int* __restrict__ active_iters,
                                                            double* __restrict__ ws, int* __restrict__ ok) {
  extern __shared__ __attribute__((aligned(16))) double sm_p4pf[];
  const size_t hyp = blockIdx.x;
  const int p = (int)(hyp / B), b = (int)(hyp % B);
  if (b >= active_iters[p]) { if (threadIdx.x == 0) ok[hyp] = 0; return; }
  const bool good = p4pfdev::p4pf_action_wg(data + (size_t)offsets[p] * 5, samples + hyp * 4, sm_p4pf, ws + hyp * kFpWs);
  if (threadIdx.x == 0) ok[hyp] = good ? 1 : 0;
}

__global__ __launch_bounds__(64) void k_p4pf_c(int nprob, int B, const int* __restrict__ active_iters, const double* __restrict__ ws,
                                               const double* __restrict__ sol, const int* __restrict__ solmask, double* __restrict__ models,
                                               int* __restrict__ counts, int* __restrict__ dense_count, int* __restrict__ tags,
                                               int* __restrict__ hyp_base) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  const int p = blockIdx.y;
  if (b >= B || p >= nprob) return;
  const size_t hyp = (size_t)p * B + b;
  if (b >= active_iters[p]) { counts[hyp] = 0; return; }
  const int mask = solmask[hyp];
  if (!mask) { counts[hyp] = 0; return; }
  double N[p4pfdev::kNorm];
  for (int k = 0; k < p4pfdev::kNorm; ++k) N[k] = ws[hyp * kFpWs + k];
  double mloc[10 * 12];
  int nm = 0;
  for (int i = 0; i < 10; ++i) {
    if (!((mask >> i) & 1)) continue;
    const double* v = sol + (hyp * 10 + i) * 5;
    const double w = v[4] / v[0];
    if (!(w >= 0.0)) continue;   // negative or NaN focal length^2 (four_point_focal_length_helper.cc:917-921)
    p4pfdev::projection_from_solution(N, w, v[3] / v[0], v[2] / v[0], v[1] / v[0], mloc + 12 * nm);
    nm++;
  }
  counts[hyp] = nm;
  if (nm == 0) return;
  const int mm = 10;
  const int base = atomicAdd(&dense_count[p], nm);
  hyp_base[hyp] = base;
  double* mo = models + ((size_t)p * B * mm + base) * (size_t)kStride;
  int* tg = tags + (size_t)p * B * mm + base;
  for (int j = 0; j < nm; ++j) {
    for (int k = 0; k < 12; ++k) mo[j * kStride + k] = mloc[j * 12 + k];
    for (int k = 12; k < kStride; ++k) mo[j * kStride + k] = 0.0;
    tg[j] = b * mm + j;
  }
}

// ---- homography hypotheses in three stages (as SQPnP: the 9 x 9 Jacobi SVD of A^T A was 2.3 KB of dynamically indexed
// per-lane arrays in scratch, 49 ns per hypothesis): M, T1, T2 per thread -> svd9_team with V -> H per thread.
// ws per hypothesis: [M 81 | T1 9 | T2 9 | Hn 9]
constexpr int kHomWs = 108;
__global__ __launch_bounds__(64) void k_hom_a(int nprob, int B, const int64_t* __restrict__ offsets, const double* __restrict__ data,
                                              const int* __restrict__ samples, const int* __restrict__ active_iters,
                                              double* __restrict__ ws) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  const int p = blockIdx.y;
  if (b >= B || p >= nprob || b >= active_iters[p]) return;
  const size_t hyp = (size_t)p * B + b;
  const double* pd = data + (size_t)offsets[p] * 4;
  double subset[16], M[81], T1[9], T2[9];
  for (int i = 0; i < 4; ++i) {
    const int idx = samples[hyp * 4 + i];
    for (int k = 0; k < 4; ++k) subset[i * 4 + k] = pd[(size_t)idx * 4 + k];
  }
  rsc::four_point_homography_pre(subset, M, T1, T2);
  double* w = ws + hyp * kHomWs;
  for (int k = 0; k < 81; ++k) w[k] = M[k];
  for (int k = 0; k < 9; ++k) { w[81 + k] = T1[k]; w[90 + k] = T2[k]; }
}
__global__ __launch_bounds__(64) void k_hom_b(size_t nhyp, int B, const int* __restrict__ active_iters, double* __restrict__ ws) {
  __shared__ double lds[kSqTeamsPerWave][81 + 81 + 81 + 9];   // W | U | V | S
  const int team = threadIdx.x / kSqTeam, tl = threadIdx.x % kSqTeam;
  if (team >= kSqTeamsPerWave) return;
  const size_t hyp = (size_t)blockIdx.x * kSqTeamsPerWave + team;
  if (hyp >= nhyp || (int)(hyp % B) >= active_iters[hyp / B]) return;
  double* W = lds[team]; double* U = W + 81; double* V = U + 81; double* S = V + 81;
  double* w = ws + hyp * kHomWs;
  rsc::svd9_team<kSqTeam>(w, W, U, S, tl, V);
  for (int e = tl; e < 9; e += kSqTeam) w[99 + e] = V[9 * e + 8];   // the last right singular vector
}
__global__ __launch_bounds__(64) void k_hom_c(int nprob, int B, const int* __restrict__ active_iters, const double* __restrict__ ws,
                                              double* __restrict__ models, int* __restrict__ counts, int* __restrict__ dense_count,
                                              int* __restrict__ tags, int* __restrict__ hyp_base) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  const int p = blockIdx.y;
  if (b >= B || p >= nprob) return;
  const size_t hyp = (size_t)p * B + b;
  if (b >= active_iters[p]) { counts[hyp] = 0; return; }
  const double* w = ws + hyp * kHomWs;
  double Hn[9], T1[9], T2[9], H[9];
  for (int k = 0; k < 9; ++k) { T1[k] = w[81 + k]; T2[k] = w[90 + k]; Hn[k] = w[99 + k]; }
  rsc::four_point_homography_post(Hn, T1, T2, H);
  counts[hyp] = 1;
  const int base = atomicAdd(&dense_count[p], 1);
  hyp_base[hyp] = base;
  double* mo = models + ((size_t)p * B + base) * (size_t)kStride;   // max_models = 1
  for (int k = 0; k < 9; ++k) mo[k] = H[k];
  for (int k = 9; k < kStride; ++k) mo[k] = 0.0;
  tags[(size_t)p * B + base] = b;
}

// ---- DLS-PnP hypotheses (estimate_calibrated_absolute_pose.cc:89-97): stage A = dls_kernels.hip (launch_dls_stage_a), then the
// eigen stage below.
__global__ __launch_bounds__(64) void k_dls_b(int nprob, int B, const int64_t* __restrict__ offsets,
                                              const double* __restrict__ data, const int* __restrict__ samples,
                                              const int* __restrict__ active_iters, const double* __restrict__ action,
                                              const double* __restrict__ tfac, const int* __restrict__ okflag,
                                              double* __restrict__ models, int* __restrict__ counts,
                                              int* __restrict__ dense_count, int* __restrict__ tags, int* __restrict__ hyp_base) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  const int p = blockIdx.y;
  if (b >= B || p >= nprob) return;
  const size_t hyp = (size_t)p * B + b;
  if (b >= active_iters[p]) { counts[hyp] = 0; return; }
  int nm = 0;
  double quats[4 * dlsdev::kMaxSolutions], ts[3 * dlsdev::kMaxSolutions];
  if (okflag[hyp]) {
    double H[729], V[729], tf[27];
    const double* a = action + hyp * 729;
    for (int k = 0; k < 729; ++k) H[k] = a[k];
    for (int k = 0; k < 27; ++k) tf[k] = tfac[hyp * 27 + k];
    const double* pd = data + (size_t)offsets[p] * 5;
    nm = dlsdev::stage_b(H, V, tf, 3, pd + 2, 5, samples + hyp * 3, quats, ts);
  }
  counts[hyp] = nm;
  if (nm == 0) return;
  const int mm = dlsdev::kMaxSolutions;
  const int base = atomicAdd(&dense_count[p], nm);
  hyp_base[hyp] = base;
  double* mo = models + ((size_t)p * B * mm + base) * (size_t)kStride;
  int* tg = tags + (size_t)p * B * mm + base;
  for (int j = 0; j < nm; ++j) {
    double R[9];
    rsc::quat_to_rot(quats + 4 * j, R);
    const double* t = ts + 3 * j;
    double* m = mo + (size_t)j * kStride;
    for (int k = 0; k < 9; ++k) m[k] = R[k];
    for (int c = 0; c < 3; ++c) m[9 + c] = -((R[c] * t[0] + R[3 + c] * t[1]) + R[6 + c] * t[2]);
    for (int k = 12; k < kStride; ++k) m[k] = 0.0;
    tg[j] = b * mm + j;
  }
}

// stage B on chip: a team of 32 lanes per hypothesis, H / V / X in LDS (eig_team.h), lanes 0..26 turn one eigenvector
// column each into a pose, kept in column order by a team prefix sum
#ifndef THIP_DLS_TEAM
#define THIP_DLS_TEAM 32
#endif
constexpr int kDlsTeam = THIP_DLS_TEAM, kDlsColRounds = (27 + kDlsTeam - 1) / kDlsTeam, kDlsTeamsPerWave = 64 / kDlsTeam, kDlsTeamLds = 729 + 27 * dlsdev::kKeptRows + 81;   // H | kept rows of V | wr, wi, ort
__global__ __launch_bounds__(64) void k_dls_b_team(size_t nhyp, int B, const int64_t* __restrict__ offsets,
                                                   const double* __restrict__ data, const int* __restrict__ samples,
                                                   const int* __restrict__ active_iters, double* __restrict__ action,
                                                   const double* __restrict__ tfac, const int* __restrict__ okflag,
                                                   double* __restrict__ models, int* __restrict__ counts,
                                                   int* __restrict__ dense_count, int* __restrict__ tags, int* __restrict__ hyp_base) {
  __shared__ double lds[kDlsTeamsPerWave][kDlsTeamLds];
  const int team = threadIdx.x / kDlsTeam, tl = threadIdx.x % kDlsTeam;
  const size_t hyp = (size_t)blockIdx.x * kDlsTeamsPerWave + team;
  if (hyp >= nhyp) return;
  const int p = (int)(hyp / B), b = (int)(hyp % B);
  if (b >= active_iters[p] || !okflag[hyp]) { if (tl == 0) counts[hyp] = 0; return; }
  // The kernel is bound by the matrices resident per CU (one dependent chain each), i.e. by LDS per matrix.  H stays in
  // LDS; the work array X of the back-substitution lives in the hypothesis' own action-matrix slot in HBM (free once H is
  // on chip); so does the full eigenvector matrix while the Householder reflectors are accumulated -- after that only the
  // four rows column_solution() reads are carried (eig_team.h, NR): 14.7 instead of 24.6 KB of LDS per wave = ten
  // instead of six resident waves per CU
  double* H = lds[team]; double* Vk = H + 729; double* wr = Vk + 27 * dlsdev::kKeptRows; double* wi = wr + 27; double* ort = wi + 27;
  double* a = action + hyp * 729;
  for (int e = tl; e < 729; e += kDlsTeam) H[e] = a[e];
  rsc::team_sync();
  int nn = 27;
  asm volatile("" : "+s"(nn));   // the order stays a run-time value: with the literal the loops unroll into 250 VGPRs (two waves per SIMD)
  const bool good = rsc::eig_team<kDlsTeam, true, dlsdev::kKeptRows>(nn, H, a, a, wr, wi, ort, tl, Vk, dlsdev::kKeptRow);
  // the 27 eigenvector columns by lane (kDlsColRounds rounds of the team), the poses kept in column order by team prefix sums
  double quat[kDlsColRounds][4], tr[kDlsColRounds][3];
  int rank[kDlsColRounds];
  int nm = 0;
#pragma unroll
  for (int rd = 0; rd < kDlsColRounds; ++rd) {
    const int col = tl + rd * kDlsTeam;
    bool keep = false;
    if (good && col < 27) {
      const double* pd = data + (size_t)offsets[p] * 5;
      keep = dlsdev::column_solution<true>(Vk, wi, col, tfac + hyp * 27, 3, pd + 2, 5, samples + hyp * 3, quat[rd], tr[rd]);
    }
    int incl = keep ? 1 : 0;
    for (int o = 1; o < kDlsTeam; o <<= 1) { const int v = __shfl_up(incl, o, kDlsTeam); if (tl >= o) incl += v; }
    rank[rd] = keep ? nm + incl - 1 : -1;
    nm += __shfl(incl, kDlsTeam - 1, kDlsTeam);
  }
  int base = 0;
  if (tl == 0) { counts[hyp] = nm; if (nm) { base = atomicAdd(&dense_count[p], nm); hyp_base[hyp] = base; } }
  base = __shfl(base, 0, kDlsTeam);
#pragma unroll
  for (int rd = 0; rd < kDlsColRounds; ++rd) {
    if (rank[rd] < 0) continue;
    const int mm = dlsdev::kMaxSolutions, j = rank[rd];
    double* m = models + ((size_t)p * B * mm + base + j) * (size_t)kStride;
    double R[9];
    rsc::quat_to_rot(quat[rd], R);
    for (int k = 0; k < 9; ++k) m[k] = R[k];
    for (int c = 0; c < 3; ++c) m[9 + c] = -((R[c] * tr[rd][0] + R[3 + c] * tr[rd][1]) + R[6 + c] * tr[rd][2]);
    for (int k = 12; k < kStride; ++k) m[k] = 0.0;
    tags[(size_t)p * B * mm + base + j] = b * mm + j;
  }
}

__global__ __launch_bounds__(64) void k_gdls_b_team(size_t nhyp, int B, const int64_t* __restrict__ offsets,
                                                    const double* __restrict__ data, const int* __restrict__ samples,
                                                    const int* __restrict__ active_iters, double* __restrict__ action,
                                                    const double* __restrict__ tfac, const int* __restrict__ okflag,
                                                    double* __restrict__ models, int* __restrict__ counts,
                                                    int* __restrict__ dense_count, int* __restrict__ tags, int* __restrict__ hyp_base) {
  __shared__ double lds[kDlsTeamsPerWave][kDlsTeamLds];
  const int team = threadIdx.x / kDlsTeam, tl = threadIdx.x % kDlsTeam;
  const size_t hyp = (size_t)blockIdx.x * kDlsTeamsPerWave + team;
  if (hyp >= nhyp) return;
  const int p = (int)(hyp / B), b = (int)(hyp % B);
  if (b >= active_iters[p] || !okflag[hyp]) { if (tl == 0) counts[hyp] = 0; return; }
  double* H = lds[team]; double* Vk = H + 729; double* wr = Vk + 27 * dlsdev::kKeptRows; double* wi = wr + 27; double* ort = wi + 27;
  double* a = action + hyp * 729;
  for (int e = tl; e < 729; e += kDlsTeam) H[e] = a[e];
  rsc::team_sync();
  int nn = 27;
  asm volatile("" : "+s"(nn));
  const bool good = rsc::eig_team<kDlsTeam, true, dlsdev::kKeptRows>(nn, H, a, a, wr, wi, ort, tl, Vk, dlsdev::kKeptRow);
  double quat[kDlsColRounds][4], tr[kDlsColRounds][3], sc[kDlsColRounds];
  int rank[kDlsColRounds];
  int nm = 0;
#pragma unroll
  for (int rd = 0; rd < kDlsColRounds; ++rd) {
    const int col = tl + rd * kDlsTeam;
    bool keep = false;
    sc[rd] = 0.0;
    if (good && col < 27)
      keep = dlsdev::column_solution_gdls(Vk, wi, col, tfac + hyp * 36, 4, data + (size_t)offsets[p] * kSimDatum, kSimDatum, 0, 9, 3,
                                          samples + hyp * 4, quat[rd], tr[rd], &sc[rd]);
    int incl = keep ? 1 : 0;
    for (int o = 1; o < kDlsTeam; o <<= 1) { const int v = __shfl_up(incl, o, kDlsTeam); if (tl >= o) incl += v; }
    rank[rd] = keep ? nm + incl - 1 : -1;
    nm += __shfl(incl, kDlsTeam - 1, kDlsTeam);
  }
  int base = 0;
  if (tl == 0) { counts[hyp] = nm; if (nm) { base = atomicAdd(&dense_count[p], nm); hyp_base[hyp] = base; } }
  base = __shfl(base, 0, kDlsTeam);
#pragma unroll
  for (int rd = 0; rd < kDlsColRounds; ++rd) {
    if (rank[rd] < 0) continue;
    const int mm = dlsdev::kMaxSolutions, j = rank[rd];
    double* m = models + ((size_t)p * B * mm + base + j) * (size_t)kStride;
    double Rs[9];
    rsc::quat_to_rot(quat[rd], Rs);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) m[3 * r + c] = Rs[3 * c + r];                              // rotation = R^T
    for (int r = 0; r < 3; ++r) m[9 + r] = (m[3 * r] * -tr[rd][0] + m[3 * r + 1] * -tr[rd][1]) + m[3 * r + 2] * -tr[rd][2];       // rotation * -t
    m[12] = sc[rd];
    for (int k = 13; k < kStride; ++k) m[k] = 0.0;
    tags[(size_t)p * B * mm + base + j] = b * mm + j;
  }
}

// DlsPnp on problems of any size (the directly bound solver, sfm.cc:577): stage A per workgroup (dls_kernels.hip), then a thread per problem
__global__ __launch_bounds__(64) void k_dls_solve_b(int num, const int64_t* __restrict__ offsets, const double* __restrict__ world,
                                                    const double* __restrict__ action, const double* __restrict__ tfac,
                                                    const int* __restrict__ okflag, double* __restrict__ quats,
                                                    double* __restrict__ ts, int* __restrict__ nsol) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num) return;
  double q[4 * dlsdev::kMaxSolutions], t[3 * dlsdev::kMaxSolutions];
  int n = 0;
  if (okflag[i]) {
    double H[729], V[729], tf[27];
    for (int k = 0; k < 729; ++k) H[k] = action[(size_t)i * 729 + k];
    for (int k = 0; k < 27; ++k) tf[k] = tfac[(size_t)i * 27 + k];
    const int64_t o = offsets[i];
    n = dlsdev::stage_b(H, V, tf, (int)(offsets[i + 1] - o), world + 3 * o, 3, nullptr, q, t);
  }
  nsol[i] = n;
  for (int k = 0; k < 4 * dlsdev::kMaxSolutions; ++k) quats[(size_t)i * 4 * dlsdev::kMaxSolutions + k] = (k < 4 * n) ? q[k] : 0.0;
  for (int k = 0; k < 3 * dlsdev::kMaxSolutions; ++k) ts[(size_t)i * 3 * dlsdev::kMaxSolutions + k] = (k < 3 * n) ? t[k] : 0.0;
}

// the index tables of the polynomial system live in constant memory, built once per process
// k_p4pf_a needs 70 KB of dynamic LDS (above the 64 KB default)
int p4pf_kernel_ready() {
  static std::once_flag once;
  static int status = 0;
  std::call_once(once, [] {
    const hipError_t e = hipFuncSetAttribute((const void*)k_p4pf_a, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p4pfdev::kLdsBytes);
    if (e != hipSuccess) status = set_error(THEIA_HIP_ERR_NO_DEVICE, hipGetErrorString(e));
  });
  return status;
}

// ------------------------------------------------------------------ host side
// Host-side loops over independent problems (sample streams, acceptance replay) on the library's persistent team of host
// threads (host_team.h: starting and joining 16 threads per loop cost ~0.6 ms, a round has two such loops), four problems
// per thread at least.
template <class F>
void host_parallel_for(int n, F&& fn) {
  host_for(n, std::min<unsigned>(host_thread_cap(), (unsigned)std::max(1, n / 4)), fn);
}

double ms_between(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
  return std::chrono::duration<double, std::milli>(b - a).count();
}

// The correspondences on the device.  They come from pageable memory: the copy occupies the calling thread for
// total * ds * 8 B / ~11 GB/s (6 ms for 1000 pairs x 2000 matches).  It runs on a helper thread while the caller draws the
// first chunk's sample streams.  Before wait() the caller enqueues only the two hipMemsetAsync of its set-up (the UPnP
// states, the best models), which touch neither this buffer nor anything that reads it; the pointer is handed out by data()
// alone, which joins the helper first, so nothing that reads the buffer can be enqueued ahead of the copy.
class Correspondences {
  DBuf<double> buf;
  std::thread th;
  hipError_t err = hipSuccess;
  void join() { if (th.joinable()) th.join(); }

 public:
  ~Correspondences() { join(); }
  int start(const double* src, size_t count, hipStream_t st) {
    if (int rc = buf.ensure(count)) return rc;
    double* dst = buf.p; const size_t bytes = sizeof(double) * count;
    int dev = 0;
    (void)hipGetDevice(&dev);
    try {
      th = std::thread([this, src, dst, bytes, st, dev] { (void)hipSetDevice(dev); err = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st); });
    } catch (...) {   // no thread to be had: the same copy, here
      err = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
    }
    return 0;
  }
  int wait() {
    join();
    return err == hipSuccess ? 0 : set_error(THEIA_HIP_ERR_INTERNAL, "upload of the correspondences: %s", hipGetErrorString(err));
  }
  const double* data() { join(); return buf.p; }
};

struct FitScoreEvents {   // start of the fit, between fit and score, end of the score
  hipEvent_t ev0 = nullptr, ev1 = nullptr, evm = nullptr;
  int create() { HIP_TRYR(hipEventCreate(&ev0)); HIP_TRYR(hipEventCreate(&ev1)); HIP_TRYR(hipEventCreate(&evm)); return 0; }
  ~FitScoreEvents() { for (hipEvent_t e : {ev0, ev1, evm}) if (e) (void)hipEventDestroy(e); }
};

// The sample streams of the NEXT chunk's first round are drawn while this chunk's kernels run; their 30 MB go up on
// the copy stream at once, into the device buffer of their host buffer, and the solver stream waits for the event instead
// of copying them between two chunks' kernels.
struct PreUpload {
  hipEvent_t ev = nullptr; bool pending = false;
  PreUpload() { (void)hipEventCreateWithFlags(&ev, hipEventDisableTiming); }
  ~PreUpload() { if (ev) { if (pending) (void)hipEventSynchronize(ev); (void)hipEventDestroy(ev); } }   // (the buffers outlive the copy)
};

struct LoEvent { int prob, slot, hyp; int samples[8]; };   // hyp: (problem in chunk) * B + iteration of the round, or -1

// one round of one chunk
struct Round {
  int c0, cn, B = 0;
  size_t nh = 0;             // cn * B hypotheses
  bool samples_up = false;   // the samples went up on the copy stream already
  std::chrono::steady_clock::time_point tp0, tp1, tp2;
};

// One call of the batch driver: its buffers, what it knows about the estimator, and the stages of a round in the order
// ransac_run() calls them.
struct RansacCall {
  const theia_ransac_batch* const batch;
  const theia_ransac_params& P;
  theia_ransac_result* const result;
  const StreamInit* const si;
  // development switches, read once per call
  const bool fit_one_kernel = getenv("THEIA_HIP_FIT_ONE_KERNEL") != nullptr, dls_thread_eig = getenv("THEIA_HIP_DLS_THREAD_EIG") != nullptr,
             debug = getenv("THEIA_HIP_RANSAC_DEBUG") != nullptr, refit = getenv("THEIA_HIP_RANSAC_REFIT") != nullptr,
             host_timing = getenv("THEIA_HIP_RANSAC_TIMING") != nullptr;
  std::chrono::steady_clock::time_point t_entry, t_loop;

  // ---- traits of the estimator and the sampler (check())
  int est = 0, nprob = 0, m = 0, ds = 0, kMaxModels = 0;
  EstParams ep{0.0, 0.0};
  bool gdls_est = false, dls_est = false, trivial_refine = false, rel_pose = false, uncal_pose = false, homog = false, fund = false,
       lmed = false, upnp_est = false, p4pfr_est = false, p4pfr_first_call = false;
  double p4pfr_limits[4] = {0.0, 0.0, 0.0, 0.0};
  theia_ba_options lo_opts;
  double log_failure_prob = 0.0;

  SolverCall call;   // (ahead of every buffer)
  hipStream_t st = nullptr, copy_st = nullptr;
  FitScoreEvents clk;
  double fit_ms = 0.0, score_ms = 0.0, fit_score_ms = 0.0;

  // ---- sizes (setup())
  int64_t total = 0;
  int nmax = 0, first_round = 0, chunk = 0;
  static constexpr int next_round = 1024;
  std::vector<uint8_t> undersized;
  size_t lmed_lds = 0, lds_bytes = 0;
  int lmed_in_lds = 1;
  bool use_lds = false;

  // ---- buffers
  Correspondences corr; DBuf<int64_t> d_off;
  DBuf<int> d_samples2[2], d_counts, d_ninl, d_active, d_best_samples, d_best_slot, d_dense, d_tags;   // d_samples2: by host sample buffer
  DBuf<int> d_hyp_base;   // [problem][iteration] first dense model of the hypothesis (k_fit)
  DBuf<int> d_save;       // {problem, hypothesis, slot} triples of k_save_best
  DBuf<double> d_models, d_cost, d_best_models;
  DBuf<double> d_pcost; DBuf<int> d_pninl, d_prefix;   // the round's scores packed for the download (k_pack_scores)
  DBuf<double> d_dls_action, d_dls_tfac, d_dls_u; DBuf<int> d_dls_ok, d_iter_base;   // DLS: stage A -> stage B
  DBuf<double> d_fp_ws, d_fp_sol; DBuf<int> d_fp_ok, d_fp_mask;   // five-point: stages a -> b -> c
  std::vector<double> h_dls_u; dls::GlibcRand dls_gen; std::vector<int> h_iter_base;
  DBuf<uint8_t> d_mask;
  HBuf<double> h_rot2[2];   // P4Pfr: the "random rotation" matrix of every hypothesis of a round (made where its draws are taken)
  DBuf<double> d_rot;
  HBuf<int> h_samples2[2], h_counts, h_ninl, h_active2[2];   // pinned: sources / destinations of the per-round transfers (samples / active
                                                             // counts twice: the next chunk's first round is drawn while the GPU works)
  HBuf<double> h_cost;
  HBuf<int> h_hyp_base, h_prefix;   // per hypothesis: first model in its problem's dense order; per problem: first packed score
  DBuf<double> d_upnp_state;   // UPnP: the estimator's accumulating cost parameters per problem (upnp_kernels.hip)
  std::vector<ProblemState> S;
  std::vector<StreamRound> SR;
  std::vector<dls::GlibcRand> SD;   // streams: every problem's own rand() stream (DLS / gDLS)
  // LO-RANSAC (absolute / relative pose): batched RefineModel over a list of events
  DBuf<int> d_ev_prob, d_ev_samples, d_ev_slot, d_ev_hyp, d_ev_count, d_ev_success, d_lo_model_id;
  DBuf<int64_t> d_ev_off;
  DBuf<double> d_ev_model, d_ev_cam, d_lo_uv, d_lo_X, d_cur_models, d_lo_intr, d_ev_sqt;
  DBuf<char> d_lo_out;

  // ---- the chunk loop's state
  int bufi = 0, pre_c0 = -1, pre_B = 0;   // pre_*: the first round of chunk pre_c0 already sits in buffer 1 - bufi
  bool offsets_up = false;
  PreUpload pre_up;

  RansacCall(const theia_ransac_batch* b, const theia_ransac_params& p, theia_ransac_result* r, const StreamInit* s)
      : batch(b), P(p), result(r), si(s) {}

  int check();
  void set_lo_options();
  int setup();
  int gen_round(int c0, int cn, bool first, int buf, int* B_out);
  int begin_round(Round& r, bool first);
  int upload_round(Round& r);
  int launch_fit_dls(const Round& r);
  int launch_fit(const Round& r);
  int launch_score(const Round& r);
  int predraw_next_chunk(const Round& r);
  int download_scores(Round& r);
  int run_lo(const std::vector<LoEvent>& evs, int round_B, std::vector<int>& success);
  int replay(const Round& r);
  int save_best(const Round& r);
  int upload_offsets();
  int finish();
};

// Argument and estimator checks; the traits.  nprob == 0 afterwards: nothing to do.
int RansacCall::check() {
  // SampleConsensusEstimator ctor CHECKs (sample_consensus_estimator.h:217-223)
  if (!(P.error_thresh > 0)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "Error threshold must be set to greater than zero");
  if (!(P.min_inlier_ratio <= 1.0) || !(P.min_inlier_ratio >= 0.0)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "min_inlier_ratio must be in [0, 1]");
  if (!(P.failure_probability < 1.0) || !(P.failure_probability > 0.0)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "failure_probability must be in (0, 1)");
  if (P.max_iterations < P.min_iterations) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "max_iterations < min_iterations");
  est = batch->estimator;
  if (est == THEIA_EST_UNCALIBRATED_RELATIVE_POSE && !batch->estimator_params)
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "the uncalibrated relative-pose estimator needs estimator_params = {min, max focal length}");
  if (est == THEIA_EST_UNCALIBRATED_RELATIVE_POSE && batch->estimator_params) {
    ep.min_focal = batch->estimator_params[0];
    ep.max_focal = batch->estimator_params[1];
  }
  gdls_est = est == THEIA_EST_SIMILARITY_2D3D;
  dls_est = est == THEIA_EST_ABSOLUTE_POSE_DLS || gdls_est;   // the Macaulay pipeline: stage A -> eigen stage
  if (est < 0 || est > THEIA_EST_CAMERA_ALIGNMENT) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "unknown estimator id");
  // estimators that keep Estimator::RefineModel's default "return true" (solvers/estimator.h:86-88): LO only counts
  trivial_refine = est == THEIA_EST_ESSENTIAL_MATRIX || est == THEIA_EST_DOMINANT_PLANE ||
                   est == THEIA_EST_RELATIVE_POSE_KNOWN_ORIENTATION || est == THEIA_EST_ABSOLUTE_POSE_KNOWN_ORIENTATION ||
                   est == THEIA_EST_TRIANGULATION || est == THEIA_EST_RADIAL_HOMOGRAPHY || est == THEIA_EST_SIMILARITY_2D3D ||
                   est == THEIA_EST_UNCALIBRATED_ABSOLUTE_POSE || est == THEIA_EST_RIGID_TRANSFORMATION_2D3D ||
                   est == THEIA_EST_RADIAL_DIST_UNCALIBRATED_ABSOLUTE_POSE || est == THEIA_EST_CAMERA_ALIGNMENT;
  rel_pose = est == THEIA_EST_RELATIVE_POSE; uncal_pose = est == THEIA_EST_UNCALIBRATED_RELATIVE_POSE;
  homog = est == THEIA_EST_HOMOGRAPHY; fund = est == THEIA_EST_FUNDAMENTAL_MATRIX;
  // every estimator's RefineModel is built: BundleAdjustView (absolute pose), BundleAdjustTwoViewsAngular ((un)calibrated
  // relative pose), OptimizeHomography, OptimizeFundamentalMatrix, and the default "return true" of the rest
  // exhaustive_sampler.cc:49-51 CHECK
  if (P.ransac_type == THEIA_RANSAC_EXHAUSTIVE && sample_size(est) != 2)
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "ExhaustiveSampler makes a hard assumption that the number of samples needed is 2.");
  lmed = P.ransac_type == THEIA_RANSAC_LMED;
  if (P.ransac_type != THEIA_RANSAC_RANSAC && P.ransac_type != THEIA_RANSAC_PROSAC && !lmed &&
      P.ransac_type != THEIA_RANSAC_EXHAUSTIVE)
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "unknown ransac_type");
  nprob = batch->num_problems;
  if (nprob < 0 || (nprob > 0 && (!batch->offsets || !batch->data))) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "bad batch");
  int rc = check_result_arrays(nprob, result);
  if (rc) return rc;
  reset_counters(result);
  if (nprob == 0) return 0;
  if ((rc = call.open())) return rc;
  st = call.st;
  if (dls_est && (rc = dls_ensure_tables())) return rc;
  upnp_est = est == THEIA_EST_RIGID_TRANSFORMATION_2D3D;
  if (upnp_est && (rc = upnp_ensure_tables())) return rc;
  // P4Pfr: estimator_params = RadialDistUncalibratedAbsolutePoseMetaData {max focal length, min focal length, max distortion, min
  // distortion} [, first call of the process (the solver's static generator re-seeds the shared stream with 42)]
  p4pfr_est = est == THEIA_EST_RADIAL_DIST_UNCALIBRATED_ABSOLUTE_POSE;
  if (p4pfr_est) {
    if (!batch->estimator_params)
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "the radial-distortion absolute-pose estimator needs estimator_params = {max focal length, min focal length, max distortion, min distortion, first call (0 / 1)}");
    for (int k = 0; k < 4; ++k) p4pfr_limits[k] = batch->estimator_params[k];
    p4pfr_first_call = !si && batch->estimator_params[4] != 0.0;   // (streams: per problem, StreamInit::p4pfr_first)
    if ((rc = p4pfr_check_limits(p4pfr_limits))) return rc;
    if (P.ransac_type == THEIA_RANSAC_EXHAUSTIVE) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "the exhaustive sampler draws pairs: sample size 4 does not fit");
    if ((rc = p4pfr_ensure_tables())) return rc;
  }
  t_entry = std::chrono::steady_clock::now();
  m = sample_size(est); ds = datum_size(est);
  kMaxModels = max_models(est);   // slot stride of this estimator
  log_failure_prob = std::log(P.failure_probability);
  return 0;
}

// the options of every estimator's RefineModel
void RansacCall::set_lo_options() {
  theia_ba_options_default(&lo_opts);
  lo_opts.max_num_iterations = 2;                        // estimate_calibrated_absolute_pose.cc:124-129
  lo_opts.use_homogeneous_point_parametrization = 0;
  lo_opts.intrinsics_to_optimize = THEIA_INTR_NONE;
  lo_opts.loss_function_type = THEIA_LOSS_HUBER;
  lo_opts.robust_loss_width = P.error_thresh * 1.5;
  lo_opts.use_inner_iterations = 0;
  if (rel_pose || homog) {                               // estimate_relative_pose.cc:120-126, estimate_homography.cc:94-98
    lo_opts.max_num_iterations = 15;
    lo_opts.loss_function_type = THEIA_LOSS_TRUNCATED;
    lo_opts.robust_loss_width = P.error_thresh;
  }
  if (fund) { lo_opts.max_num_iterations = 2; lo_opts.loss_function_type = THEIA_LOSS_TRIVIAL; }   // estimate_fundamental_matrix.cc:56-57
  if (uncal_pose) lo_opts.max_num_iterations = 10;      // estimate_uncalibrated_relative_pose.cc:162-165 (HUBER, 1.5 x thresh)
}

// sizes, the upload of the correspondences, LDS opt-ins, problem states
int RansacCall::setup() {
  int rc;
  total = batch->offsets[nprob];
  undersized.assign(nprob, 0);
  for (int p = 0; p < nprob; ++p) {
    const int64_t n = batch->offsets[p + 1] - batch->offsets[p];
    if (n <= 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "Cannot perform estimation with 0 data measurements!");
    // fewer data than the minimal sample: the reference's sampler cannot be initialised for this problem (CHECK).  In a
    // batch only that problem fails (success = 0, no inliers, zero model); the others run.
    if (n < m) undersized[p] = 1;
    if (n > (1 << 30)) return set_error(THEIA_HIP_ERR_UNSUPPORTED, "problem too large");
    nmax = std::max(nmax, (int)n);
  }
  if ((rc = clk.create())) return rc;
  if ((rc = corr.start(batch->data, (size_t)total * ds, st)) || (rc = d_off.ensure(nprob + 1))) return rc;

  // round size: everything at once when the iteration count is fixed/small,
  // otherwise chunks that the adaptive bound usually ends within
  first_round = std::max(128, std::min(P.max_iterations, std::max(P.min_iterations, 512)));
  first_round = std::min(first_round, 4096);
  // problems per chunk: bound the model workspace (3 GiB by default -- 1.5 GiB cost five-point 1.4 % and SQPnP 5 % in per-chunk
  // synchronisations; THEIA_HIP_RANSAC_WORKSPACE_MB overrides)
  const size_t per_hyp = (size_t)kMaxModels * kStride * sizeof(double);
  static const size_t ws_bytes = [] { const char* e = getenv("THEIA_HIP_RANSAC_WORKSPACE_MB"); return e && atol(e) > 0 ? (size_t)atol(e) << 20 : (size_t)3 << 30; }();
  chunk = (int)std::max<size_t>(1, ws_bytes / (per_hyp * (size_t)first_round));
  chunk = std::min(chunk, nprob);

  lmed_lds = (size_t)nmax * sizeof(double);
  if (lmed) {
    // the squared residuals of a model stay in LDS for the radix select: 160 KB per workgroup on gfx950, 8 KB kept for the rest;
    // beyond that (more than 19 456 data in a problem) the passes of the select re-evaluate them (lmed_sq)
    if (lmed_lds > 152 * 1024) { lmed_lds = 0; lmed_in_lds = 0; }
    if (lmed_lds > 48 * 1024) {
      HIP_TRYR(hipFuncSetAttribute((const void*)k_score_lmed, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lmed_lds));
      HIP_TRYR(hipFuncSetAttribute((const void*)k_inlier_mask_lmed, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lmed_lds));
      HIP_TRYR(hipFuncSetAttribute((const void*)k_lo_lmed_bound, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lmed_lds));
    }
  }
  use_lds = (size_t)nmax * ds * sizeof(double) <= 96 * 1024;
  lds_bytes = use_lds ? (size_t)nmax * ds * sizeof(double) : 0;
  if (use_lds && lds_bytes > 48 * 1024) {
    // every instance that can be launched below opts in (the compile-time-estimator instances are kernels of their own)
    const void* fn = (const void*)k_score<true>;
    if (est == THEIA_EST_RELATIVE_POSE) fn = (const void*)k_score<true, THEIA_EST_RELATIVE_POSE>;
    else if (est == THEIA_EST_ESSENTIAL_MATRIX) fn = (const void*)k_score<true, THEIA_EST_ESSENTIAL_MATRIX>;
    else if (est == THEIA_EST_ABSOLUTE_POSE_KNEIP) fn = (const void*)k_score<true, THEIA_EST_ABSOLUTE_POSE_KNEIP>;
    else if (est == THEIA_EST_ABSOLUTE_POSE_DLS) fn = (const void*)k_score<true, THEIA_EST_ABSOLUTE_POSE_DLS>;
    else if (est == THEIA_EST_ABSOLUTE_POSE_SQPNP) fn = (const void*)k_score<true, THEIA_EST_ABSOLUTE_POSE_SQPNP>;
    HIP_TRYR(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  }

  if (upnp_est) {
    if ((rc = d_upnp_state.ensure((size_t)nprob * upnp_state_doubles()))) return rc;
    HIP_TRYR(hipMemsetAsync(d_upnp_state.p, 0, sizeof(double) * (size_t)nprob * upnp_state_doubles(), st));
  }
  S.resize(nprob);
  SR.resize(si ? nprob : 0);
  SD.resize(si && si->dls_start ? nprob : 0);
  host_parallel_for(nprob, [&](int p) {   // (the generator's 624-word seeding and the index permutation of every problem: ~1 us each)
    ProblemState& s = S[p];
    if (si) s.rng = si->gen[si->stream[p]];
    else s.rng.seed(batch->seeds ? batch->seeds[p] : P.seed + (uint32_t)p);
    s.p4pfr_first = si ? si->p4pfr_first[si->stream[p]] != 0 : p4pfr_first_call;
    s.last_k = 0;
    if (si && si->dls_start) SD[p] = si->dls_start[si->stream[p]];
    problem_init(s, (int)(batch->offsets[p + 1] - batch->offsets[p]), m, P, log_failure_prob, undersized[p] != 0);
  });
  if (P.use_lo && (rc = d_cur_models.ensure((size_t)nprob * kStride))) return rc;
  if ((rc = d_best_models.ensure((size_t)nprob * kStride))) return rc;
  HIP_TRYR(hipMemsetAsync(d_best_models.p, 0, sizeof(double) * nprob * kStride, st));
  copy_st = copy_stream();
  t_loop = std::chrono::steady_clock::now();
  return 0;
}

// one round of a chunk on the host, into host buffer `buf`: iterations per problem and the sample streams
// (gen_round_problem); problems are independent (own generator, own slice): host threads share them
int RansacCall::gen_round(int c0, int cn, bool first, int buf, int* B_out) {
  HBuf<int>& act = h_active2[buf]; HBuf<int>& smp = h_samples2[buf]; HBuf<double>& rotb = h_rot2[buf];
  int B = 0;
  if (!act.assign(cn, 0)) return set_error(THEIA_HIP_ERR_OUT_OF_MEMORY, "hipHostMalloc failed");
  for (int q = 0; q < cn; ++q) {
    ProblemState& s = S[c0 + q];
    s.round_iters = 0;
    if (s.done) continue;
    const int cap = first ? first_round : next_round;
    s.round_iters = std::min(cap, s.max_iterations - s.it);
    act[q] = s.round_iters;
    B = std::max(B, s.round_iters);
  }
  *B_out = B;
  if (B == 0) return 0;
  if (!smp.resize((size_t)cn * B * m)) return set_error(THEIA_HIP_ERR_OUT_OF_MEMORY, "hipHostMalloc failed");
  if (p4pfr_est && !rotb.resize((size_t)cn * B * 9)) return set_error(THEIA_HIP_ERR_OUT_OF_MEMORY, "hipHostMalloc failed");
  host_parallel_for(cn, [&](int q) {
    ProblemState& s = S[c0 + q];
    double* rot = p4pfr_est ? rotb.data() + (size_t)q * B * 9 : nullptr;   // the three draws of a hypothesis land in its matrix' slot
    gen_round_problem(s, si ? &SR[c0 + q] : nullptr, P.ransac_type, m, B, p4pfr_est, smp.data() + (size_t)q * B * m, rot, 9);
    for (int b = 0; p4pfr_est && b < s.round_iters; ++b) {
      const double v[3] = {rot[(size_t)b * 9], rot[(size_t)b * 9 + 1], rot[(size_t)b * 9 + 2]};
      p4pfr_rotation_from_draws(v, rot + (size_t)b * 9);
    }
  });
  return 0;
}

// the round's samples: the ones drawn ahead for this chunk, or drawn now
int RansacCall::begin_round(Round& r, bool first) {
  r.tp0 = std::chrono::steady_clock::now();
  if (first && pre_c0 == r.c0) { bufi ^= 1; r.B = pre_B; pre_c0 = -1; r.samples_up = pre_up.pending; }
  else if (int rc = gen_round(r.c0, r.cn, first, bufi, &r.B)) return rc;
  r.nh = (size_t)r.cn * r.B;
  r.tp1 = std::chrono::steady_clock::now();
  return 0;
}

int RansacCall::upload_offsets() {
  if (int rc = corr.wait()) return rc;
  HIP_TRYR(hipMemcpyAsync(d_off.p, batch->offsets, sizeof(int64_t) * (nprob + 1), hipMemcpyHostToDevice, st));
  offsets_up = true;
  return 0;
}

// the round's device buffers, samples and active counts; starts the fit's clock
int RansacCall::upload_round(Round& r) {
  int rc;
  const size_t nh = r.nh;
  const int cn = r.cn;
  DBuf<int>& d_samples = d_samples2[bufi];
  if ((rc = d_samples.ensure(nh * m)) || (rc = d_counts.ensure(nh)) || (rc = d_models.ensure(nh * kMaxModels * kStride)) ||
      (rc = d_cost.ensure(nh * kMaxModels)) || (rc = d_ninl.ensure(nh * kMaxModels)) || (rc = d_active.ensure(cn)) ||
      (rc = d_dense.ensure(cn)) || (rc = d_tags.ensure(nh * kMaxModels)) || (rc = d_hyp_base.ensure(nh)))
    return rc;
  if (!offsets_up && (rc = upload_offsets())) return rc;
  HIP_TRYR(hipMemsetAsync(d_dense.p, 0, sizeof(int) * cn, st));
  if (r.samples_up) { HIP_TRYR(hipStreamWaitEvent(st, pre_up.ev, 0)); pre_up.pending = false; }
  else HIP_TRYR(hipMemcpyAsync(d_samples.p, h_samples2[bufi].data(), sizeof(int) * nh * m, hipMemcpyHostToDevice, st));
  HIP_TRYR(hipMemcpyAsync(d_active.p, h_active2[bufi].data(), sizeof(int) * cn, hipMemcpyHostToDevice, st));
  HIP_TRYR(hipEventRecord(clk.ev0, st));
  return 0;
}

// DLS / gDLS: the Macaulay terms of the round's calls, stage A (dls_kernels.hip), eigen stage
int RansacCall::launch_fit_dls(const Round& r) {
  int rc;
  const int c0 = r.c0, cn = r.cn, B = r.B;
  const size_t nh = r.nh;
  const int* d_samples = d_samples2[bufi].p;
  const double* d_data = corr.data();
  h_iter_base.assign(cn, 0);
  size_t had = h_dls_u.size();
  if (si) {   // streams: every problem's calls continue its own rand() stream -- this round's terms, problem after problem
    h_dls_u.clear(); had = (size_t)-1;
    for (int q = 0; q < cn; ++q) {
      ProblemState& s = S[c0 + q];
      h_iter_base[q] = (int)(h_dls_u.size() / 4);
      for (int k = 0; k < 4 * s.round_iters; ++k) h_dls_u.push_back(dls::macaulay_term_from_rand(SD[c0 + q].next()));
    }
  } else {
    int calls = 0;
    for (int q = 0; q < cn; ++q) { h_iter_base[q] = S[c0 + q].it; calls = std::max(calls, S[c0 + q].it + S[c0 + q].round_iters); }
    dls::dls_terms(h_dls_u, dls_gen, (size_t)calls);
  }
  if ((rc = d_dls_action.ensure(nh * 729)) || (rc = d_dls_tfac.ensure(nh * 36)) || (rc = d_dls_ok.ensure(nh)) ||
      (rc = d_iter_base.ensure(cn)))
    return rc;
  if (h_dls_u.size() != had || d_dls_u.cap < h_dls_u.size()) {
    if ((rc = d_dls_u.ensure(std::max<size_t>(h_dls_u.size(), 4 * 4096)))) return rc;
    HIP_TRYR(hipMemcpyAsync(d_dls_u.p, h_dls_u.data(), sizeof(double) * h_dls_u.size(), hipMemcpyHostToDevice, st));
  }
  HIP_TRYR(hipMemcpyAsync(d_iter_base.p, h_iter_base.data(), sizeof(int) * cn, hipMemcpyHostToDevice, st));
  HIP_TRYR(hipEventRecord(clk.ev0, st));   // (re-recorded: the uploads above are not part of the fit time)
  launch_dls_stage_a(gdls_est, gdls_est ? kSimDatum : 5, cn, B, d_off.p + c0, d_data, d_samples, d_active.p, d_iter_base.p, d_dls_u.p,
                     d_dls_action.p, d_dls_tfac.p, d_dls_ok.p, st);
  const unsigned team_grid = (unsigned)((nh + kDlsTeamsPerWave - 1) / kDlsTeamsPerWave);
  if (gdls_est)
    k_gdls_b_team<<<team_grid, 64, 0, st>>>(nh, B, d_off.p + c0, d_data, d_samples, d_active.p, d_dls_action.p, d_dls_tfac.p, d_dls_ok.p,
                                            d_models.p, d_counts.p, d_dense.p, d_tags.p, d_hyp_base.p);
  else if (dls_thread_eig)
    k_dls_b<<<dim3((B + 63) / 64, cn), 64, 0, st>>>(cn, B, d_off.p + c0, d_data, d_samples, d_active.p, d_dls_action.p, d_dls_tfac.p,
                                                    d_dls_ok.p, d_models.p, d_counts.p, d_dense.p, d_tags.p, d_hyp_base.p);
  else
    k_dls_b_team<<<team_grid, 64, 0, st>>>(nh, B, d_off.p + c0, d_data, d_samples, d_active.p, d_dls_action.p, d_dls_tfac.p, d_dls_ok.p,
                                           d_models.p, d_counts.p, d_dense.p, d_tags.p, d_hyp_base.p);
  return 0;
}

// the minimal solver of the estimator on every hypothesis of the round; ends the fit's clock
int RansacCall::launch_fit(const Round& r) {
  int rc;
  const int c0 = r.c0, cn = r.cn, B = r.B;
  const size_t nh = r.nh;
  const int* d_samples = d_samples2[bufi].p;
  const double* d_data = corr.data();
  const int64_t* off = d_off.p + c0;
  const dim3 grid((B + 63) / 64, cn);
  if (dls_est) {
    if ((rc = launch_fit_dls(r))) return rc;
  } else if ((est == THEIA_EST_RELATIVE_POSE || est == THEIA_EST_ESSENTIAL_MATRIX) && !fit_one_kernel) {
    if ((rc = d_fp_ws.ensure(nh * kFpWs)) || (rc = d_fp_sol.ensure(nh * 40)) || (rc = d_fp_ok.ensure(nh)) || (rc = d_fp_mask.ensure(nh)))
      return rc;
    k_fit5_a_team<<<(unsigned)((nh + 3) / 4), 64, 0, st>>>(cn, B, off, d_data, d_samples, d_active.p, d_fp_ws.p, d_fp_ok.p);
    k_fit5_b<false><<<(unsigned)((nh + kFpTeamsPerWave - 1) / kFpTeamsPerWave), 64, 0, st>>>(nh, d_fp_ok.p, d_fp_ws.p, d_fp_sol.p, d_fp_mask.p);
    // (one LANE per root on teams of 16 -- a lane carries one model instead of ten -- measured 8 % slower on the leg: two or
    // three of a hypothesis' ten roots are real, so most lanes of such a team idle)
    if (est == THEIA_EST_RELATIVE_POSE)
      k_fit5_c<THEIA_EST_RELATIVE_POSE><<<grid, 64, 0, st>>>(cn, B, off, d_data, d_samples, d_active.p, d_fp_ws.p, d_fp_sol.p,
                                                            d_fp_mask.p, d_models.p, d_counts.p, d_dense.p, d_tags.p, d_hyp_base.p);
    else
      k_fit5_c<THEIA_EST_ESSENTIAL_MATRIX><<<grid, 64, 0, st>>>(cn, B, off, d_data, d_samples, d_active.p, d_fp_ws.p, d_fp_sol.p,
                                                               d_fp_mask.p, d_models.p, d_counts.p, d_dense.p, d_tags.p, d_hyp_base.p);
  } else if (p4pfr_est) {
    if ((rc = d_fp_ws.ensure(nh * (size_t)p4pfr_workspace_doubles())) || (rc = d_rot.ensure(nh * 9))) return rc;
    HIP_TRYR(hipMemcpyAsync(d_rot.p, h_rot2[bufi].data(), sizeof(double) * nh * 9, hipMemcpyHostToDevice, st));
    HIP_TRYR(hipEventRecord(clk.ev0, st));   // (re-recorded: the upload above is not part of the fit time)
    launch_p4pfr_fit(cn, B, off, d_data, d_samples, d_active.p, d_rot.p, p4pfr_limits, d_fp_ws.p, d_models.p, d_counts.p, d_dense.p,
                     d_tags.p, d_hyp_base.p, st);
  } else if (upnp_est) {
    if ((rc = d_fp_ws.ensure(nh * (size_t)upnp_workspace_doubles()))) return rc;
    launch_upnp_fit(cn, B, off, d_data, d_samples, d_active.p, d_upnp_state.p + (size_t)c0 * upnp_state_doubles(), d_fp_ws.p,
                    d_models.p, d_counts.p, d_dense.p, d_tags.p, d_hyp_base.p, st);
  } else if (est == THEIA_EST_UNCALIBRATED_ABSOLUTE_POSE) {
    if ((rc = d_fp_ws.ensure(nh * kFpWs)) || (rc = d_fp_sol.ensure(nh * 50)) || (rc = d_fp_ok.ensure(nh)) || (rc = d_fp_mask.ensure(nh)))
      return rc;
    if ((rc = launch_p4pf_fit(cn, B, off, d_data, d_samples, d_active.p, d_fp_ws.p, d_fp_sol.p, d_fp_ok.p, d_fp_mask.p, d_models.p,
                              d_counts.p, d_dense.p, d_tags.p, d_hyp_base.p, st)))
      return rc;
  } else if (est == THEIA_EST_HOMOGRAPHY && !fit_one_kernel) {
    if ((rc = d_fp_ws.ensure(nh * kHomWs))) return rc;
    k_hom_a<<<grid, 64, 0, st>>>(cn, B, off, d_data, d_samples, d_active.p, d_fp_ws.p);
    k_hom_b<<<(unsigned)((nh + kSqTeamsPerWave - 1) / kSqTeamsPerWave), 64, 0, st>>>(nh, B, d_active.p, d_fp_ws.p);
    k_hom_c<<<grid, 64, 0, st>>>(cn, B, d_active.p, d_fp_ws.p, d_models.p, d_counts.p, d_dense.p, d_tags.p, d_hyp_base.p);
  } else if (est == THEIA_EST_ABSOLUTE_POSE_SQPNP && !fit_one_kernel) {
    if ((rc = d_fp_ws.ensure(nh * kSqWs)) || (rc = d_fp_ok.ensure(nh))) return rc;
    k_sqp_a<<<grid, 64, 0, st>>>(cn, B, off, d_data, d_samples, d_active.p, d_fp_ws.p, d_fp_ok.p);
    k_sqp_b<<<(unsigned)((nh + kSqTeamsPerWave - 1) / kSqTeamsPerWave), 64, 0, st>>>(nh, d_fp_ok.p, d_fp_ws.p);
    k_sqp_c<<<grid, 64, 0, st>>>(cn, B, d_active.p, d_fp_ok.p, d_fp_ws.p, d_models.p, d_counts.p, d_dense.p, d_tags.p, d_hyp_base.p);
  } else {
#define THIP_FIT(E) k_fit<E><<<grid, 64, 0, st>>>(est, cn, B, off, d_data, d_samples, d_active.p, d_models.p, d_counts.p, d_dense.p, d_tags.p, d_hyp_base.p, ep)
    switch (est) {
      case THEIA_EST_RELATIVE_POSE: THIP_FIT(THEIA_EST_RELATIVE_POSE); break;
      case THEIA_EST_ESSENTIAL_MATRIX: THIP_FIT(THEIA_EST_ESSENTIAL_MATRIX); break;
      case THEIA_EST_ABSOLUTE_POSE_KNEIP: THIP_FIT(THEIA_EST_ABSOLUTE_POSE_KNEIP); break;
      case THEIA_EST_ABSOLUTE_POSE_SQPNP: THIP_FIT(THEIA_EST_ABSOLUTE_POSE_SQPNP); break;
      case THEIA_EST_FUNDAMENTAL_MATRIX: THIP_FIT(THEIA_EST_FUNDAMENTAL_MATRIX); break;
      case THEIA_EST_HOMOGRAPHY: THIP_FIT(THEIA_EST_HOMOGRAPHY); break;
      case THEIA_EST_DOMINANT_PLANE: THIP_FIT(THEIA_EST_DOMINANT_PLANE); break;
      case THEIA_EST_RELATIVE_POSE_KNOWN_ORIENTATION: THIP_FIT(THEIA_EST_RELATIVE_POSE_KNOWN_ORIENTATION); break;
      case THEIA_EST_UNCALIBRATED_RELATIVE_POSE: THIP_FIT(THEIA_EST_UNCALIBRATED_RELATIVE_POSE); break;
      case THEIA_EST_TRIANGULATION: THIP_FIT(THEIA_EST_TRIANGULATION); break;
      case THEIA_EST_RADIAL_HOMOGRAPHY: THIP_FIT(THEIA_EST_RADIAL_HOMOGRAPHY); break;
      case THEIA_EST_CAMERA_ALIGNMENT: THIP_FIT(THEIA_EST_CAMERA_ALIGNMENT); break;
      default: THIP_FIT(THEIA_EST_ABSOLUTE_POSE_KNOWN_ORIENTATION); break;
    }
#undef THIP_FIT
  }
  HIP_TRYR(hipEventRecord(clk.evm, st));
  return 0;
}

// every correspondence of a problem under every model of its hypotheses; ends the score's clock
int RansacCall::launch_score(const Round& r) {
  const int c0 = r.c0, cn = r.cn, B = r.B;
  const double* d_data = corr.data();
  if (lmed) {
    dim3 grid(B * kMaxModels, cn);
    k_score_lmed<<<grid, 256, lmed_lds, st>>>(est, cn, B, d_off.p + c0, d_data, d_models.p, d_dense.p, d_tags.p, d_cost.p, d_ninl.p, lmed_in_lds);
  } else {
#define THIP_SCORE(L, E, BYTES) k_score<L, E><<<dim3((B * kMaxModels + score_threads(E) - 1) / score_threads(E), cn), score_threads(E), BYTES, st>>>(est, cn, B, d_off.p + c0, d_data, d_models.p, d_dense.p, d_tags.p, P.error_thresh, P.use_mle, d_cost.p, d_ninl.p)
    if (use_lds) {
      if (est == THEIA_EST_RELATIVE_POSE) THIP_SCORE(true, THEIA_EST_RELATIVE_POSE, lds_bytes);
      else if (est == THEIA_EST_ESSENTIAL_MATRIX) THIP_SCORE(true, THEIA_EST_ESSENTIAL_MATRIX, lds_bytes);
      else if (est == THEIA_EST_ABSOLUTE_POSE_KNEIP) THIP_SCORE(true, THEIA_EST_ABSOLUTE_POSE_KNEIP, lds_bytes);
      else if (est == THEIA_EST_ABSOLUTE_POSE_DLS) THIP_SCORE(true, THEIA_EST_ABSOLUTE_POSE_DLS, lds_bytes);
      else if (est == THEIA_EST_ABSOLUTE_POSE_SQPNP) THIP_SCORE(true, THEIA_EST_ABSOLUTE_POSE_SQPNP, lds_bytes);
      else THIP_SCORE(true, -1, lds_bytes);
    } else {
      if (est == THEIA_EST_RELATIVE_POSE) THIP_SCORE(false, THEIA_EST_RELATIVE_POSE, 0);
      else if (est == THEIA_EST_ABSOLUTE_POSE_SQPNP) THIP_SCORE(false, THEIA_EST_ABSOLUTE_POSE_SQPNP, 0);
      else THIP_SCORE(false, -1, 0);
    }
#undef THIP_SCORE
  }
  HIP_TRYR(hipEventRecord(clk.ev1, st));
  return 0;
}

// while the GPU fits and scores this round: the first round of the next chunk (its problems are not touched before)
int RansacCall::predraw_next_chunk(const Round& r) {
  if (!(pre_c0 < 0 && r.c0 + chunk < nprob)) return 0;
  int rc;
  const int nc0 = r.c0 + chunk, ncn = std::min(chunk, nprob - nc0), nb = 1 - bufi;
  if ((rc = gen_round(nc0, ncn, true, nb, &pre_B))) return rc;
  pre_c0 = nc0;
  const size_t pnh = (size_t)ncn * pre_B;
  if (pre_B > 0 && copy_st && pre_up.ev && !pre_up.pending) {
    if ((rc = d_samples2[nb].ensure(pnh * m))) return rc;
    HIP_TRYR(hipMemcpyAsync(d_samples2[nb].p, h_samples2[nb].data(), sizeof(int) * pnh * m, hipMemcpyHostToDevice, copy_st));
    HIP_TRYR(hipEventRecord(pre_up.ev, copy_st));
    pre_up.pending = true;
  }
  return 0;
}

// model counts down, then the scores packed: only the models that exist travel (all max_models slots of every hypothesis
// were 100 - 270 MB a round)
int RansacCall::download_scores(Round& r) {
  int rc;
  const int cn = r.cn, B = r.B;
  const size_t nh = r.nh;
  if (!h_counts.resize(nh) || !h_hyp_base.resize(nh) || !h_prefix.resize((size_t)cn + 1))
    return set_error(THEIA_HIP_ERR_OUT_OF_MEMORY, "hipHostMalloc failed");
  HIP_TRYR(hipMemcpyAsync(h_counts.data(), d_counts.p, sizeof(int) * nh, hipMemcpyDeviceToHost, st));
  HIP_TRYR(hipMemcpyAsync(h_hyp_base.data(), d_hyp_base.p, sizeof(int) * nh, hipMemcpyDeviceToHost, st));
  HIP_TRYR(hipMemcpyAsync(h_prefix.data() + 1, d_dense.p, sizeof(int) * cn, hipMemcpyDeviceToHost, st));
  HIP_TRYR(hipGetLastError());
  if ((rc = predraw_next_chunk(r))) return rc;
  HIP_TRYR(call.wait());
  h_prefix.data()[0] = 0;
  int most = 0;
  for (int q = 0; q < cn; ++q) { most = std::max(most, h_prefix.data()[q + 1]); h_prefix.data()[q + 1] += h_prefix.data()[q]; }
  const size_t total_models = (size_t)h_prefix.data()[cn];
  if (!h_cost.resize(std::max<size_t>(1, total_models)) || !h_ninl.resize(std::max<size_t>(1, total_models)))
    return set_error(THEIA_HIP_ERR_OUT_OF_MEMORY, "hipHostMalloc failed");
  if (total_models > 0) {
    if ((rc = d_prefix.ensure((size_t)cn + 1)) || (rc = d_pcost.ensure(total_models)) || (rc = d_pninl.ensure(total_models))) return rc;
    HIP_TRYR(hipMemcpyAsync(d_prefix.p, h_prefix.data(), sizeof(int) * ((size_t)cn + 1), hipMemcpyHostToDevice, st));
    k_pack_scores<<<dim3((unsigned)std::min(64, (most + 255) / 256), cn), 256, 0, st>>>(B, kMaxModels, d_dense.p, d_prefix.p, d_cost.p, d_ninl.p,
                                                                                    d_pcost.p, d_pninl.p);
    HIP_TRYR(hipMemcpyAsync(h_cost.data(), d_pcost.p, sizeof(double) * total_models, hipMemcpyDeviceToHost, st));
    HIP_TRYR(hipMemcpyAsync(h_ninl.data(), d_pninl.p, sizeof(int) * total_models, hipMemcpyDeviceToHost, st));
    HIP_TRYR(hipGetLastError());
    HIP_TRYR(call.wait());
  }
  r.tp2 = std::chrono::steady_clock::now();
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, clk.ev0, clk.ev1) == hipSuccess) fit_score_ms += ms;
  if (hipEventElapsedTime(&ms, clk.ev0, clk.evm) == hipSuccess) fit_ms += ms;
  if (hipEventElapsedTime(&ms, clk.evm, clk.ev1) == hipSuccess) score_ms += ms;
  return 0;
}

// refines every event's model on its inliers; writes the refined pose to d_cur_models[prob]
int RansacCall::run_lo(const std::vector<LoEvent>& evs, int round_B, std::vector<int>& success) {
  const int nev = (int)evs.size();
  success.assign(nev, 0);
  if (nev == 0) return 0;
  const double* d_data = corr.data();
  std::vector<int> hp(nev), hs((size_t)nev * kMaxSample), hsl(nev), hmod(nev, THEIA_CAM_PINHOLE), hhyp(nev);
  std::vector<int64_t> hoff(nev + 1, 0);
  std::vector<double> hintr((size_t)nev * THEIA_MAX_INTRINSICS, 0.0);
  for (int e = 0; e < nev; ++e) {
    hp[e] = evs[e].prob; hsl[e] = evs[e].slot; hhyp[e] = evs[e].hyp;
    for (int k = 0; k < kMaxSample; ++k) hs[(size_t)e * kMaxSample + k] = evs[e].samples[k];
    hoff[e + 1] = hoff[e] + S[evs[e].prob].n;          // capacity: every datum could be an inlier
    hintr[(size_t)e * THEIA_MAX_INTRINSICS] = 1.0; hintr[(size_t)e * THEIA_MAX_INTRINSICS + 1] = 1.0;   // Camera(): f = 1, aspect 1
  }
  int rc2;
  if ((rc2 = d_ev_prob.ensure(nev)) || (rc2 = d_ev_samples.ensure((size_t)nev * kMaxSample)) || (rc2 = d_ev_slot.ensure(nev)) ||
      (rc2 = d_ev_count.ensure(nev)) || (rc2 = d_ev_success.ensure(nev)) || (rc2 = d_ev_off.ensure(nev + 1)) ||
      (rc2 = d_ev_model.ensure((size_t)nev * kStride)) || (rc2 = d_ev_cam.ensure((size_t)nev * 9)) ||
      (rc2 = d_lo_uv.ensure((size_t)hoff[nev] * 2)) || (rc2 = d_lo_X.ensure((size_t)hoff[nev] * 4)) ||
      (rc2 = d_lo_intr.ensure(hintr.size())) || (rc2 = d_lo_model_id.ensure(nev)) ||
      (rc2 = d_lo_out.ensure(views_batch_out_bytes() * nev)))
    return rc2;
  HIP_TRYR(hipMemcpyAsync(d_ev_prob.p, hp.data(), sizeof(int) * nev, hipMemcpyHostToDevice, st));
  HIP_TRYR(hipMemcpyAsync(d_ev_samples.p, hs.data(), sizeof(int) * nev * kMaxSample, hipMemcpyHostToDevice, st));
  HIP_TRYR(hipMemcpyAsync(d_ev_slot.p, hsl.data(), sizeof(int) * nev, hipMemcpyHostToDevice, st));
  if ((rc2 = d_ev_hyp.ensure(nev))) return rc2;
  HIP_TRYR(hipMemcpyAsync(d_ev_hyp.p, hhyp.data(), sizeof(int) * nev, hipMemcpyHostToDevice, st));
  HIP_TRYR(hipMemcpyAsync(d_ev_off.p, hoff.data(), sizeof(int64_t) * (nev + 1), hipMemcpyHostToDevice, st));
  HIP_TRYR(hipMemcpyAsync(d_lo_intr.p, hintr.data(), sizeof(double) * hintr.size(), hipMemcpyHostToDevice, st));
  HIP_TRYR(hipMemcpyAsync(d_lo_model_id.p, hmod.data(), sizeof(int) * nev, hipMemcpyHostToDevice, st));
  k_lo_prepare<<<(nev + 63) / 64, 64, 0, st>>>(est, nev, d_ev_prob.p, d_ev_samples.p, d_ev_slot.p, d_ev_hyp.p, round_B,
                                               d_models.p, d_hyp_base.p, d_off.p, d_data,
                                               d_cur_models.p, d_ev_model.p, d_ev_cam.p, ep);
  if (lmed) {
    if ((rc2 = d_ev_sqt.ensure(nev))) return rc2;
    k_lo_lmed_bound<<<nev, 256, lmed_lds, st>>>(est, d_ev_prob.p, d_off.p, d_data, d_ev_model.p, d_ev_sqt.p, lmed_in_lds);
  }
  k_lo_gather<<<nev, 64, 0, st>>>(est, d_ev_prob.p, d_off.p, d_data, d_ev_model.p, P.error_thresh, lmed ? d_ev_sqt.p : nullptr, d_ev_off.p, d_ev_count.p,
                                  reinterpret_cast<double2*>(d_lo_uv.p), reinterpret_cast<double4*>(d_lo_X.p));
  if (fund)
    fundamental_batch_device(nev, d_ev_off.p, d_ev_count.p, d_lo_X.p, d_ev_cam.p, &lo_opts, d_lo_out.p, st);
  else if (homog)
    homography_batch_device(nev, d_ev_off.p, d_ev_count.p, d_lo_X.p, d_ev_cam.p, &lo_opts, d_lo_out.p, st);
  else if (rel_pose || uncal_pose)   // the relative-pose RefineModel asks for CGNR, the uncalibrated one keeps the direct default
    twoview_batch_device(nev, d_ev_off.p, d_ev_count.p, d_lo_X.p, d_ev_cam.p, &lo_opts, rel_pose ? 1 : 0, d_lo_out.p, st);
  else
    views_batch_device(nev, d_ev_off.p, d_ev_count.p, d_lo_uv.p, nullptr, d_lo_X.p, d_ev_cam.p, d_lo_intr.p, d_lo_model_id.p,
                       nullptr, &lo_opts, d_lo_out.p, st);
  k_lo_finish<<<(nev + 63) / 64, 64, 0, st>>>(est, nev, d_ev_prob.p, d_ev_cam.p, d_ev_model.p,
                                              reinterpret_cast<const BatchLmOut*>(d_lo_out.p), d_cur_models.p, d_ev_success.p);
  HIP_TRYR(hipMemcpyAsync(success.data(), d_ev_success.p, sizeof(int) * nev, hipMemcpyDeviceToHost, st));
  HIP_TRYR(call.wait());
  return 0;
}

// Sequential replay of the acceptance rules (replay_problem).  With use_lo a problem pauses at each RefineModel event; the
// events of all problems are refined as one batch, then every replay resumes where it stopped.
int RansacCall::replay(const Round& r) {
  const int c0 = r.c0, cn = r.cn;
  for (int q = 0; q < cn; ++q) replay_begin_round(S[c0 + q]);
  const RoundScores sc{r.B, h_counts.data(), h_hyp_base.data(), h_prefix.data(), h_cost.data(), h_ninl.data(), h_samples2[bufi].data()};
  std::vector<LoEvent> events;
  std::vector<int> ev_ok;
  std::atomic<long long> n_hyp{0}, n_scored{0};
  while (true) {
    events.clear();
    // without LO nothing is shared between the problems' replays (the counters are atomics): host threads
    auto replay_one = [&](int q) {
      ProblemState& s = S[c0 + q];
      ReplaySink sink;
      replay_problem(s, q, m, sc, P, log_failure_prob, trivial_refine, sink);
      if (sink.paused) {
        LoEvent ev; ev.prob = c0 + q; ev.slot = sink.lo_slot; ev.hyp = sink.lo_hyp;
        for (int i = 0; i < kMaxSample; ++i) ev.samples[i] = s.best_samples[i];
        events.push_back(ev);
      }
      n_hyp += sink.hypotheses; n_scored += sink.models_scored;
    };
    if (P.use_lo) { for (int q = 0; q < cn; ++q) replay_one(q); }   // LO events are collected in problem order
    else host_parallel_for(cn, replay_one);
    if (events.empty()) break;
    if (int rc = run_lo(events, r.B, ev_ok)) return rc;
    for (size_t e = 0; e < events.size(); ++e) {
      ProblemState& s = S[events[e].prob];
      if (debug)
        std::fprintf(stderr, "[hip] prob %d it %d slot %d ratio %.17g lo %d\n", events[e].prob, s.base_it + s.rb, events[e].slot, s.pending_ratio, ev_ok[e]);
      replay_lo_result(s, m, ev_ok[e] != 0, P, log_failure_prob);
    }
  }
  if (host_timing)
    std::fprintf(stderr, "[theia_hip ransac] chunk %d+%d round B=%d: samples %.1f ms, upload + kernels + download %.1f ms, replay %.1f ms\n",
                 c0, cn, r.B, ms_between(r.tp0, r.tp1), ms_between(r.tp1, r.tp2), ms_between(r.tp2, std::chrono::steady_clock::now()));
  result->hypotheses_evaluated += n_hyp.load(); result->models_scored += n_scored.load();
  return 0;
}

// best models found in this round -> d_best_models
int RansacCall::save_best(const Round& r) {
  std::vector<int> sp, sh, ss;
  for (int q = 0; q < r.cn; ++q) {
    const ProblemState& s = S[r.c0 + q];
    if (s.best_hyp >= 0) { sp.push_back(r.c0 + q); sh.push_back(s.best_hyp); ss.push_back(s.best_slot); }
  }
  if (sp.empty()) return 0;
  const int ns = (int)sp.size();
  if (int rc = d_save.ensure((size_t)3 * ns)) return rc;
  HIP_TRYR(hipMemcpyAsync(d_save.p, sp.data(), sizeof(int) * ns, hipMemcpyHostToDevice, st));
  HIP_TRYR(hipMemcpyAsync(d_save.p + ns, sh.data(), sizeof(int) * ns, hipMemcpyHostToDevice, st));
  HIP_TRYR(hipMemcpyAsync(d_save.p + 2 * ns, ss.data(), sizeof(int) * ns, hipMemcpyHostToDevice, st));
  k_save_best<<<(ns * kStride + 255) / 256, 256, 0, st>>>(est, ns, d_save.p, d_save.p + ns, d_save.p + 2 * ns, r.B, d_models.p,
                                                          d_hyp_base.p, d_best_models.p);
  HIP_TRYR(call.wait());   // the host vectors above are the sources of asynchronous uploads
  return 0;
}

// final models, inlier masks, the last LO pass, results, stream states
int RansacCall::finish() {
  int rc;
  const auto t_final = std::chrono::steady_clock::now();
  if (!offsets_up && (rc = upload_offsets())) return rc;   // (no round ran at all)
  const double* d_data = corr.data();
  std::vector<int> best_samples_all((size_t)nprob * kMaxSample, 0), best_slot_all(nprob, -1);
  for (int p = 0; p < nprob; ++p) {
    best_slot_all[p] = S[p].best_slot;
    for (int k = 0; k < kMaxSample; ++k) best_samples_all[(size_t)p * kMaxSample + k] = S[p].best_samples[k];
  }
  if ((rc = d_best_samples.ensure((size_t)nprob * kMaxSample)) || (rc = d_best_slot.ensure(nprob)) ||
      (rc = d_best_models.ensure((size_t)nprob * kStride)) || (rc = d_mask.ensure((size_t)total)))
    return rc;
  HIP_TRYR(hipMemcpyAsync(d_best_samples.p, best_samples_all.data(), sizeof(int) * nprob * kMaxSample, hipMemcpyHostToDevice, st));
  HIP_TRYR(hipMemcpyAsync(d_best_slot.p, best_slot_all.data(), sizeof(int) * nprob, hipMemcpyHostToDevice, st));
  // d_best_models already holds every problem's best model (k_save_best); THEIA_HIP_RANSAC_REFIT=1 recomputes them from the
  // best samples instead (the same bits: the solver is deterministic)
  if (refit && !dls_est)
    k_refit<<<(nprob + 63) / 64, 64, 0, st>>>(est, nprob, d_off.p, d_data, d_best_samples.p, d_best_slot.p, d_best_models.p, ep);
  std::vector<int> use_cur;   // source of an asynchronous upload: lives until the final synchronisation
  if (P.use_lo && !trivial_refine) {   // the best model of a problem may be the refined pose of its last LO event
    use_cur.resize(nprob);
    for (int p = 0; p < nprob; ++p) use_cur[p] = (S[p].best_refined && S[p].best_slot >= 0) ? 1 : 0;
    if ((rc = d_ev_slot.ensure(nprob))) return rc;
    HIP_TRYR(hipMemcpyAsync(d_ev_slot.p, use_cur.data(), sizeof(int) * nprob, hipMemcpyHostToDevice, st));
    k_select_models<<<(nprob + 63) / 64, 64, 0, st>>>(nprob, d_ev_slot.p, d_cur_models.p, d_best_models.p);
  }
  if (lmed) {
    k_inlier_mask_lmed<<<nprob, 256, lmed_lds, st>>>(est, nprob, d_off.p, d_data, d_best_models.p, d_mask.p, lmed_in_lds);
  } else {
    dim3 grid((nmax + 255) / 256, nprob);
    k_inlier_mask<<<grid, 256, 0, st>>>(est, nprob, d_off.p, d_data, d_best_models.p, P.error_thresh, d_mask.p);
  }
  if (P.use_lo && trivial_refine) {   // :401-406 with RefineModel = "return true": the counter only
    for (int p = 0; p < nprob; ++p) S[p].num_lo++;   // "++summary->num_lo_iterations" is unconditional
  } else if (P.use_lo) {   // sample_consensus_estimator.h:401-406: one more RefineModel on the final inliers (result unused)
    HIP_TRYR(hipMemcpyAsync(d_cur_models.p, d_best_models.p, sizeof(double) * nprob * kStride, hipMemcpyDeviceToDevice, st));
    std::vector<LoEvent> evs;
    for (int p = 0; p < nprob; ++p)
      if (S[p].best_slot >= 0) { LoEvent ev; ev.prob = p; ev.slot = -1; ev.hyp = -1; for (int k = 0; k < kMaxSample; ++k) ev.samples[k] = 0; evs.push_back(ev); }
    std::vector<int> ok;
    if ((rc = run_lo(evs, 0, ok))) return rc;
    for (int p = 0; p < nprob; ++p) S[p].num_lo++;   // unconditional in the reference, also when no model was found
    HIP_TRYR(hipMemcpyAsync(d_best_models.p, d_cur_models.p, sizeof(double) * nprob * kStride, hipMemcpyDeviceToDevice, st));
  }
  HIP_TRYR(hipGetLastError());
  HIP_TRYR(call.wait());
  // caller-owned (pageable) destinations: blocking copies after the stream has drained
  HIP_TRYR(hipMemcpy(result->models, d_best_models.p, sizeof(double) * nprob * kStride, hipMemcpyDeviceToHost));
  HIP_TRYR(hipMemcpy(result->inlier_mask, d_mask.p, (size_t)total, hipMemcpyDeviceToHost));
  const int used = model_doubles(est);   // the slots of a model row past the estimator's layout (theia_hip.h) are padding: handed back as zeros
  for (int p = 0; p < nprob; ++p) {
    for (int k = used; k < kStride; ++k) result->models[(size_t)p * kStride + k] = 0.0;
    const ProblemState& s = S[p];
    int cnt = 0;
    for (int64_t i = batch->offsets[p]; i < batch->offsets[p + 1]; ++i) cnt += result->inlier_mask[i];
    result->num_inliers[p] = cnt;
    result->num_iterations[p] = s.it;
    if (result->num_lo_iterations) result->num_lo_iterations[p] = s.num_lo;
    result->success[p] = 1;
    const double inlier_ratio = (double)cnt / s.n;
    result->confidence[p] = 1.0 - std::pow(1.0 - std::pow(inlier_ratio, (double)m), (double)s.it);
    if (undersized[p]) {
      result->success[p] = 0; result->num_inliers[p] = 0; result->confidence[p] = 0.0;
      for (int64_t i = batch->offsets[p]; i < batch->offsets[p + 1]; ++i) result->inlier_mask[i] = 0;
    }
  }
  result->time_fit_score_seconds = fit_score_ms * 1e-3;
  result->time_fit_seconds = fit_ms * 1e-3; result->time_score_seconds = score_ms * 1e-3;
  if (si) {   // the generator after exactly num_iterations samples: the last round's start, advanced by the words its finished iterations took
    host_parallel_for(nprob, [&](int p) {   // (a discard may regenerate the 624 words: ~3 us a problem)
      const ProblemState& s = S[p];
      if (s.it == 0) return;   // undersized, or no iteration at all: nothing drawn
      Mt19937& g = si->gen[si->stream[p]];
      g = SR[p].anchor;
      g.discard(s.last_k > 0 ? SR[p].cum[s.last_k - 1] : 0);
    });
  }
  if (host_timing)
    std::fprintf(stderr, "[theia_hip ransac] call: set-up %.1f ms, rounds %.1f ms, best models + inlier masks + results %.1f ms\n",
                 ms_between(t_entry, t_loop), ms_between(t_loop, t_final), ms_between(t_final, std::chrono::steady_clock::now()));
  return 0;
}

}  // namespace

hipStream_t solver_stream() {
  static hipStream_t s = [] {
    hipStream_t x = nullptr;
    if (hipStreamCreateWithFlags(&x, hipStreamNonBlocking) != hipSuccess) x = nullptr;
    return x;
  }();
  return s;
}
hipStream_t copy_stream() {
  static hipStream_t s = [] {
    hipStream_t x = nullptr;
    if (hipStreamCreateWithFlags(&x, hipStreamNonBlocking) != hipSuccess) x = nullptr;
    return x;
  }();
  return s;
}

int p4pf_workspace_doubles() { return kFpWs; }
int launch_p4pf_fit(int nprob, int B, const int64_t* offsets, const double* data, const int* samples, const int* active_iters,
                    double* ws, double* sol, int* ok, int* mask, double* models, int* counts, int* dense_count, int* tags,
                    int* hyp_base, hipStream_t st) {
  if (int rc = p4pf_kernel_ready()) return rc;
  const size_t nh = (size_t)nprob * B;
  k_p4pf_a<<<(unsigned)nh, p4pfdev::kThreads, p4pfdev::kLdsBytes, st>>>(nprob, B, offsets, data, samples, active_iters, ws, ok);
  k_fit5_b<true><<<(unsigned)((nh + kFpTeamsPerWave - 1) / kFpTeamsPerWave), 64, 0, st>>>(nh, ok, ws, sol, mask);
  k_p4pf_c<<<dim3((B + 63) / 64, nprob), 64, 0, st>>>(nprob, B, active_iters, ws, sol, mask, models, counts, dense_count, tags, hyp_base);
  return 0;
}
void launch_five_point(int num, const double* corr, double* E, int* nsol, hipStream_t st) {
  k_five_point<<<(num + 63) / 64, 64, 0, st>>>(num, corr, E, nsol);
}
void launch_p3p(int num, const double* corr, double* R, double* t, int* nsol, hipStream_t st) {
  k_p3p<<<(num + 63) / 64, 64, 0, st>>>(num, corr, R, t, nsol);
}
void launch_sqpnp(int num, const int64_t* offsets, const double* feat, const double* world, double* quat, double* trans, int* nsol,
                  hipStream_t st) {
  k_sqpnp<<<(num + 63) / 64, 64, 0, st>>>(num, offsets, feat, world, quat, trans, nsol);
}
void launch_dls_solve_b(int num, const int64_t* offsets, const double* world, const double* action, const double* tfac, const int* ok,
                        double* quat, double* trans, int* nsol, hipStream_t st) {
  k_dls_solve_b<<<(num + 63) / 64, 64, 0, st>>>(num, offsets, world, action, tfac, ok, quat, trans, nsol);
}

// The chunk / round loop.  Every enqueue, event record and wait of a round happens inside the stage that is named for it,
// in the order of the calls below.
int ransac_run(const theia_ransac_batch* batch, const theia_ransac_params* params, theia_ransac_result* result,
               const StreamInit* si) {
  if (!batch || !params || !result) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null argument");
  RansacCall c(batch, *params, result, si);
  int rc = c.check();
  if (rc || c.nprob == 0) return rc;
  c.set_lo_options();
  if ((rc = c.setup())) return rc;
  for (int c0 = 0; c0 < c.nprob; c0 += c.chunk) {
    const int cn = std::min(c.chunk, c.nprob - c0);
    for (bool first = true;; first = false) {
      Round r{c0, cn};
      if ((rc = c.begin_round(r, first))) return rc;
      if (r.B == 0) break;
      if ((rc = c.upload_round(r)) || (rc = c.launch_fit(r)) || (rc = c.launch_score(r)) || (rc = c.download_scores(r)) ||
          (rc = c.replay(r)) || (rc = c.save_best(r)))
        return rc;
    }
  }
  return c.finish();
}

}  // namespace thip

using namespace thip;

extern "C" {

void theia_ransac_params_default(theia_ransac_params* p) {
  // sample_consensus_estimator.h:59-68
  std::memset(p, 0, sizeof(*p));
  p->error_thresh = -1;
  p->failure_probability = 0.01;
  p->min_inlier_ratio = 0;
  p->min_iterations = 100;
  p->max_iterations = std::numeric_limits<int>::max();
  p->use_mle = 0; p->use_lo = 0; p->use_Tdd_test = 0; p->lo_start_iterations = 50;
  p->seed = 0;
}

int theia_hip_ransac_estimate_batch(const theia_ransac_batch* batch, const theia_ransac_params* params,
                                    theia_ransac_result* result) {
  return ransac_run(batch, params, result, nullptr);
}

}  // extern "C"

#ifdef THIP_EIG_STAMPS
// development: the phase stamps of eig_team (eig_team.h) summed since the last call; out[8]
extern "C" int theia_hip_debug_eig_stamps(unsigned long long* out) {
  unsigned long long zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(thip::rsc::g_eig_stamps), sizeof(zero)) != hipSuccess) return -1;
  (void)hipMemcpyToSymbol(HIP_SYMBOL(thip::rsc::g_eig_stamps), zero, sizeof(zero));
  return 0;
}
#endif
