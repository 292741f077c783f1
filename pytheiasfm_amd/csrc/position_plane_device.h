// position_plane_device.h -- the dominant plane from three points and the two known-orientation position solvers
// (relative position from two correspondences, absolute position from two rays) on the device (gfx950, FP64), one
// thread per problem.
// Built with -ffp-contract=off: the operation order below is kept identical to
// the CPU oracle's transcription of the same algorithms, which is what makes
// RANSAC inlier sets bit-identical between the two (DESIGN.md "RANSAC parity").
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>

#include "small_linalg.h"     // FullPivLU, fullpiv_lu, dswap, colpiv_qr_solve_4x3
#include "twoview_device.h"   // sampson

namespace thip {
namespace rsc {

// DominantPlaneEstimator::EstimateModel (estimate_dominant_plane_from_points.cc:62-81).
// pts: 3 x [X Y Z]; model = point(3) unit_normal(3).
RDEV bool plane_from_three_points(const double* pts, double* model) {
  const double a[3] = {pts[3] - pts[0], pts[4] - pts[1], pts[5] - pts[2]};
  const double b[3] = {pts[6] - pts[0], pts[7] - pts[1], pts[8] - pts[2]};
  const double cr[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
  const double n2 = (cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2];
  if (n2 < 1e-6) return false;
  const double nrm = sqrt(n2);
  for (int k = 0; k < 3; ++k) { model[k] = pts[k]; model[3 + k] = cr[k] / nrm; }
  return true;
}
// point-to-plane distance (:84-86; NOT squared)
RDEV double plane_error(const double* model, const double* p) {
  return fabs((model[3] * (p[0] - model[0]) + model[4] * (p[1] - model[1])) + model[5] * (p[2] - model[2]));
}

// RelativePoseFromTwoPointsWithKnownRotation
// (sfm/pose/relative_pose_from_two_points_with_known_rotation.cc:51-88):
// kernel of the 2x3 epipolar constraint, normalised.  corr: 2 x [x1 y1 x2 y2].
RDEV bool two_point_relative_position(const double* corr, double* pos) {
  double A[6];
  for (int i = 0; i < 2; ++i) {
    const double x1 = corr[4 * i], y1 = corr[4 * i + 1], x2 = corr[4 * i + 2], y2 = corr[4 * i + 3];
    A[3 * i] = -y1 + y2;
    A[3 * i + 1] = -x2 + x1;
    A[3 * i + 2] = y1 * x2 - x1 * y2;
  }
  FullPivLU f;
  fullpiv_lu(A, 2, 3, f);
  const double premult = fabs(f.maxpivot) * (DBL_EPSILON * 2.0);
  int rank = 0;
  for (int i = 0; i < f.nonzero_pivots; ++i) rank += fabs(A[i * 3 + i]) > premult;
  if (3 - rank != 1) return false;
  int cidx[3] = {0, 1, 2};
  for (int k = 0; k < f.size; ++k) dswap(cidx[k], cidx[f.colt[k]]);
  double X[2];
  X[1] = A[5] / A[4];
  X[0] = (A[2] - A[1] * X[1]) / A[0];
  double v[3] = {0.0, 0.0, 0.0};
  v[cidx[0]] = -X[0]; v[cidx[1]] = -X[1]; v[cidx[2]] = 1.0;
  const double nrm = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  for (int k = 0; k < 3; ++k) pos[k] = v[k] / nrm;
  return true;
}
// Sampson distance under E = [-position]_x (estimate_relative_pose_with_known_orientation.cc:52-58)
RDEV double known_orientation_error(const double* pos, const double* c) {
  const double E[9] = {0.0, pos[2], -pos[1], -pos[2], 0.0, pos[0], pos[1], -pos[0], 0.0};
  return sampson(E, c);
}

// PositionFromTwoRays (sfm/pose/position_from_two_rays.cc:55-83).  corr: 2 x [u v X Y Z], features
// already rotated into the world frame.
RDEV bool position_from_two_rays(const double* corr, double* pos) {
  double A[12], b[4];
  for (int i = 0; i < 2; ++i) {
    const double u = corr[5 * i], v = corr[5 * i + 1], X = corr[5 * i + 2], Y = corr[5 * i + 3], Z = corr[5 * i + 4];
    A[6 * i] = 1.0; A[6 * i + 1] = 0.0; A[6 * i + 2] = -u;
    A[6 * i + 3] = 0.0; A[6 * i + 4] = 1.0; A[6 * i + 5] = -v;
    b[2 * i] = X - u * Z; b[2 * i + 1] = Y - v * Z;
  }
  return colpiv_qr_solve_4x3(A, b, pos) == 3;
}
// AbsolutePoseWithKnownOrientationEstimator::Error (estimate_absolute_pose_with_known_orientation.cc:113-120)
RDEV double known_orientation_abs_error(const double* pos, const double* d) {
  const double px = d[2] - pos[0], py = d[3] - pos[1], pz = d[4] - pos[2];
  const double ex = px / pz - d[0], ey = py / pz - d[1];
  return ex * ex + ey * ey;
}

}  // namespace rsc
}  // namespace thip
