// alignment_device.h -- reconstruction alignment on the device (sfm/transformation/), one thread per call, over
// small_linalg.h and rotation_maps.h:
//   umeyama_finish       the tail of AlignPointCloudsUmeyamaWithWeights (align_point_clouds.cc:112-149) from the centroids, sigma
//                        and the cross-correlation: SVD of its transpose, the degenerate rule, reflection fix, scale, R, t
//   camera_alignment_fit CameraAlignmentEstimator::EstimateModel (align_reconstructions.cc:66-84): Umeyama of positions2 ->
//                        positions1 on the four sampled data, in the reference's sequential order (one lane owns the sample)
//   camera_alignment_error  CameraAlignmentEstimator::Error (:86-92)
//   similarity_apply     s * (R p) + t in the library's stated order
//   transform_camera / transform_point   TransformReconstruction's two bodies (transform_reconstruction.cc:48-67,89-91)
// Must be compiled without FMA contraction (build.sh's default): the tests restate these orders and compare bits.
#pragma once
#include "rotation_maps.h"
#include "small_linalg.h"

namespace thip {
namespace rsc {

constexpr int kAlignOk = 0, kAlignDegenerate = 1;   // THEIA_ALIGN_*

// s * (R p) + t: each row of R times p with the products added left to right, then the scale, then the translation.  The one
// order of every similarity applied in this library (similarity_error of THEIA_EST_SIMILARITY_2D3D uses it too).
RDEV void similarity_apply(const double* R, const double* t, double s, const double* p, double* out) {
  const double x = p[0], y = p[1], z = p[2];
  for (int r = 0; r < 3; ++r) out[r] = s * ((R[3 * r] * x + R[3 * r + 1] * y) + R[3 * r + 2] * z) + t[r];
}

// cc [3][3] row-major: cc[a][b] = sum_i w_i (left_i - lc)_a (right_i - rc)_b / sum w.  Writes the identity transformation and
// returns kAlignDegenerate where the reference does (:120-139: on absolute singular values).
RDEV int umeyama_finish(const double* lc, const double* rc, double sigma, const double* cc, double* R, double* t, double* scale) {
  for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
  t[0] = 0.0; t[1] = 0.0; t[2] = 0.0;
  *scale = 1.0;
  double A[9], U[9], S[3], V[9];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) A[3 * a + b] = cc[3 * b + a];   // cross_correlation.transpose()
  svd3(A, U, S, V);
  const double min_sv = fmin(S[0], fmin(S[1], S[2])), max_sv = fmax(S[0], fmax(S[1], S[2]));
  const double condition_number = max_sv / (min_sv + 1e-12);
  if (condition_number > 1e6 || min_sv < 1e-8) return kAlignDegenerate;
  double Vt[9];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) Vt[3 * a + b] = V[3 * b + a];
  const double det = det3(U) * det3(Vt);
  const double s22 = det > 0 ? 1.0 : -1.0;
  *scale = ((S[0] + S[1]) + s22 * S[2]) / sigma;
  double Us[9];
  for (int r = 0; r < 3; ++r) { Us[3 * r] = U[3 * r]; Us[3 * r + 1] = U[3 * r + 1]; Us[3 * r + 2] = U[3 * r + 2] * s22; }
  matmul3(Us, Vt, R);
  const double zero[3] = {0.0, 0.0, 0.0};
  double srl[3];
  similarity_apply(R, zero, *scale, lc, srl);   // scale * (R lc) (+ 0: exact)
  for (int r = 0; r < 3; ++r) t[r] = rc[r] - srl[r];
  return kAlignOk;
}

// subset: four data [camera1 (3) | camera2 (3)]; model: rotation (9) | translation (3) | scale.  left = camera2, right =
// camera1, unit weights (x * 1.0 is exact and left out), every sum point after point as the reference adds them.
RDEV int camera_alignment_fit(const double* subset, double* model) {
  const int n = 4;
  double lc[3] = {0.0, 0.0, 0.0}, rc[3] = {0.0, 0.0, 0.0}, wsum = 0.0;
  for (int i = 0; i < n; ++i) {
    wsum += 1.0;
    for (int k = 0; k < 3; ++k) { lc[k] += subset[6 * i + 3 + k]; rc[k] += subset[6 * i + k]; }
  }
  for (int k = 0; k < 3; ++k) { lc[k] /= wsum; rc[k] /= wsum; }
  double sigma = 0.0;
  for (int i = 0; i < n; ++i) {
    const double dx = subset[6 * i + 3] - lc[0], dy = subset[6 * i + 4] - lc[1], dz = subset[6 * i + 5] - lc[2];
    sigma += (dx * dx + dy * dy) + dz * dz;
  }
  sigma /= wsum;
  double cc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < n; ++i) {
    double dl[3], dr[3];
    for (int k = 0; k < 3; ++k) { dl[k] = subset[6 * i + 3 + k] - lc[k]; dr[k] = subset[6 * i + k] - rc[k]; }
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) cc[3 * a + b] += dl[a] * dr[b];
  }
  for (int k = 0; k < 9; ++k) cc[k] /= wsum;
  return umeyama_finish(lc, rc, sigma, cc, model, model + 9, model + 12);
}

// d: [camera1 (3) | camera2 (3)]
RDEV double camera_alignment_error(const double* m, const double* d) {
  double q[3];
  similarity_apply(m, m + 9, m[12], d + 3, q);
  const double ex = d[0] - q[0], ey = d[1] - q[1], ez = d[2] - q[2];
  return (ex * ex + ey * ey) + ez * ez;
}

// cam: position (3) | angle-axis (3), in place
RDEV void transform_camera(const double* R, const double* t, double s, double* cam) {
  double Rc[9], Rt[9], Rn[9], pos[3];
  angle_axis_to_rot(cam + 3, Rc);
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) Rt[3 * a + b] = R[3 * b + a];
  matmul3(Rc, Rt, Rn);
  rot_to_angle_axis(Rn, cam + 3);
  similarity_apply(R, t, s, cam, pos);
  cam[0] = pos[0]; cam[1] = pos[1]; cam[2] = pos[2];
}

// pt: homogeneous (4), in place
RDEV void transform_point(const double* R, const double* t, double s, double* pt) {
  const double h[3] = {pt[0] / pt[3], pt[1] / pt[3], pt[2] / pt[3]};
  double q[3];
  similarity_apply(R, t, s, h, q);
  pt[0] = q[0]; pt[1] = q[1]; pt[2] = q[2]; pt[3] = 1.0;
}

}  // namespace rsc
}  // namespace thip
