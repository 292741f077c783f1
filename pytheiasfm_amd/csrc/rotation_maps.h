// rotation_maps.h -- conversions between rotation matrices, quaternions, ceres angle-axis vectors and Eigen rotation
// vectors on the device (gfx950, FP64), and MultiplyRotations built from them.  Shared by the RANSAC solvers, the
// global-pose stages and the view-graph filters.
// Built with -ffp-contract=off: the operation order below is kept identical to
// the CPU oracle's transcription of the same algorithms, which is what makes
// RANSAC inlier sets bit-identical between the two (DESIGN.md "RANSAC parity").
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>

#include "small_linalg.h"   // RDEV

namespace thip {
namespace rsc {

// Eigen::Quaternion(Matrix3) and Quaternion::toRotationMatrix (Geometry/Quaternion.h).
// M row-major; q = [w, x, y, z].
RDEV void rot_to_quat(const double* M, double* q) {
  double t = (M[0] + M[4]) + M[8];
  if (t > 0.0) {
    t = sqrt(t + 1.0);
    q[0] = 0.5 * t;
    t = 0.5 / t;
    q[1] = (M[7] - M[5]) * t; q[2] = (M[2] - M[6]) * t; q[3] = (M[3] - M[1]) * t;
  } else {
    int i = 0;
    if (M[4] > M[0]) i = 1;
    if (M[8] > M[i * 3 + i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = sqrt(M[i * 3 + i] - M[j * 3 + j] - M[k * 3 + k] + 1.0);
    q[1 + i] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (M[k * 3 + j] - M[j * 3 + k]) * t;
    q[1 + j] = (M[j * 3 + i] + M[i * 3 + j]) * t;
    q[1 + k] = (M[k * 3 + i] + M[i * 3 + k]) * t;
  }
}
RDEV void quat_to_rot(const double* q, double* R) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
  R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
}

// ceres/rotation.h RotationMatrixToAngleAxis (via quaternion) and AngleAxisToRotationMatrix, as
// Camera::SetOrientationFromRotationMatrix / GetOrientationAsRotationMatrix use them
// (camera.cc:245-261).  R row-major.
RDEV void rot_to_angle_axis(const double* R, double* aa) {
  double q[4];
  const double trace = R[0] + R[4] + R[8];
  if (trace >= 0.0) {
    double t = sqrt(trace + 1.0);
    q[0] = 0.5 * t;
    t = 0.5 / t;
    q[1] = (R[7] - R[5]) * t; q[2] = (R[2] - R[6]) * t; q[3] = (R[3] - R[1]) * t;
  } else {
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > R[i * 3 + i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    double t = sqrt(R[i * 3 + i] - R[j * 3 + j] - R[k * 3 + k] + 1.0);
    q[i + 1] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (R[k * 3 + j] - R[j * 3 + k]) * t;
    q[j + 1] = (R[j * 3 + i] + R[i * 3 + j]) * t;
    q[k + 1] = (R[k * 3 + i] + R[i * 3 + k]) * t;
  }
  const double s2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  if (s2 > 0.0) {
    const double st = sqrt(s2), ct = q[0];
    const double two_theta = 2.0 * ((ct < 0.0) ? atan2(-st, -ct) : atan2(st, ct));
    const double k = two_theta / st;
    aa[0] = q[1] * k; aa[1] = q[2] * k; aa[2] = q[3] * k;
  } else {
    aa[0] = q[1] * 2.0; aa[1] = q[2] * 2.0; aa[2] = q[3] * 2.0;
  }
}
RDEV void angle_axis_to_rot(const double* aa, double* R) {
  const double theta2 = aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2];
  if (theta2 > DBL_EPSILON) {
    const double theta = sqrt(theta2);
    const double wx = aa[0] / theta, wy = aa[1] / theta, wz = aa[2] / theta;
    const double c = cos(theta), s = sin(theta);
    R[0] = c + wx * wx * (1.0 - c);      R[3] = wz * s + wx * wy * (1.0 - c);  R[6] = -wy * s + wx * wz * (1.0 - c);
    R[1] = wx * wy * (1.0 - c) - wz * s; R[4] = c + wy * wy * (1.0 - c);       R[7] = wx * s + wy * wz * (1.0 - c);
    R[2] = wy * s + wx * wz * (1.0 - c); R[5] = -wx * s + wy * wz * (1.0 - c); R[8] = c + wz * wz * (1.0 - c);
  } else {
    R[0] = 1.0; R[3] = aa[2]; R[6] = -aa[1];
    R[1] = -aa[2]; R[4] = 1.0; R[7] = aa[0];
    R[2] = aa[1]; R[5] = -aa[0]; R[8] = 1.0;
  }
}

// Eigen::AngleAxisd(Matrix3d) (Quaternion.h quaternionbase_assign_impl<.., 3, 3> then AngleAxis.h
// operator=(QuaternionBase)) scaled to a rotation vector, and AngleAxisd::toRotationMatrix with
// angle = |v|, axis = v / angle -- RelativePoseEstimator::RefineModel converts this way
// (estimate_relative_pose.cc:116-118,131-134; a zero vector gives NaNs there too).  R row-major.
RDEV void eigen_rot_to_rotvec(const double* R, double* v) {
  double q[4];   // x y z w
  double t = (R[0] + R[4]) + R[8];
  if (t > 0.0) {
    t = sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (R[7] - R[5]) * t; q[1] = (R[2] - R[6]) * t; q[2] = (R[3] - R[1]) * t;
  } else {
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > R[i * 3 + i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = sqrt(R[i * 3 + i] - R[j * 3 + j] - R[k * 3 + k] + 1.0);
    q[i] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (R[k * 3 + j] - R[j * 3 + k]) * t;
    q[j] = (R[j * 3 + i] + R[i * 3 + j]) * t;
    q[k] = (R[k * 3 + i] + R[i * 3 + k]) * t;
  }
  double n = sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
  double angle, axis[3];
  if (n != 0.0) {
    angle = 2.0 * atan2(n, fabs(q[3]));
    if (q[3] < 0.0) n = -n;
    axis[0] = q[0] / n; axis[1] = q[1] / n; axis[2] = q[2] / n;
  } else {
    angle = 0.0; axis[0] = 1.0; axis[1] = 0.0; axis[2] = 0.0;
  }
  v[0] = angle * axis[0]; v[1] = angle * axis[1]; v[2] = angle * axis[2];
}
RDEV void eigen_rotvec_to_rot(const double* v, double* R) {
  const double angle = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  const double ax[3] = {v[0] / angle, v[1] / angle, v[2] / angle};
  const double s = sin(angle), c = cos(angle);
  const double sa[3] = {s * ax[0], s * ax[1], s * ax[2]};
  const double ca[3] = {(1.0 - c) * ax[0], (1.0 - c) * ax[1], (1.0 - c) * ax[2]};
  double tmp;
  tmp = ca[0] * ax[1]; R[1] = tmp - sa[2]; R[3] = tmp + sa[2];
  tmp = ca[0] * ax[2]; R[2] = tmp + sa[1]; R[6] = tmp - sa[1];
  tmp = ca[1] * ax[2]; R[5] = tmp - sa[0]; R[7] = tmp + sa[0];
  R[0] = ca[0] * ax[0] + c; R[4] = ca[1] * ax[1] + c; R[8] = ca[2] * ax[2] + c;
}

}  // namespace rsc

// MultiplyRotations (math/rotation.cc:56-66), shared by the rotation stage's residual (rotation_averaging.hip) and the
// orientation filter (view_pair_filters.hip).
// MultiplyRotations(a, b): angle-axis -> matrices, product, matrix -> angle-axis (row-major matrices throughout)
__device__ __forceinline__ void multiply_rotations(const double* a, const double* b, double* out) {
  double Ra[9], Rb[9], R[9];
  rsc::angle_axis_to_rot(a, Ra);
  rsc::angle_axis_to_rot(b, Rb);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) R[3 * r + c] = (Ra[3 * r] * Rb[c] + Ra[3 * r + 1] * Rb[3 + c]) + Ra[3 * r + 2] * Rb[6 + c];
  rsc::rot_to_angle_axis(R, out);
}

}  // namespace thip
