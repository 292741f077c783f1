// radial_homography_device.h -- the six-point radial-distortion homography solver and its error on the device
// (gfx950, FP64), one thread per problem.
// Built with -ffp-contract=off: the operation order below is kept identical to
// the CPU oracle's transcription of the same algorithms, which is what makes
// RANSAC inlier sets bit-identical between the two (DESIGN.md "RANSAC parity").
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cstddef>

#include "small_linalg.h"   // right_singular_vectors, inverse3_cofactor

namespace thip {
namespace rsc {

// ------------------------------------------------------------ radial-distortion homography
// sfm/pose/six_point_radial_distortion_homography.cc:62-241, estimators/estimate_radial_distortion_homography.cc:52-111.
//
constexpr int kRadHomDatum = 12;   // [feature_left (2) | feature_right (2) | normalized left (2) | normalized right (2) | f_left f_right | lmin lmax]
// SixPointRadialDistortionHomography on six data rows; models: up to two rows of `stride` doubles
// {H (9, row-major) | l1 | l2 | H^-1 (9)}.  Returns the number of results (the reference's bool is "the quadratic had a real
// root"; solutions outside [lmin, lmax] are dropped, so zero results with a true return is possible there as well).
RDEV int radial_homography_six_point(const double* d, double* models, int stride) {
  double Mx[48], u2[6], x2[6];
  const double lmin = d[10], lmax = d[11];
  for (int i = 0; i < 6; ++i) {
    const double* r = d + kRadHomDatum * i;
    const double x0 = r[4], x1 = r[5], u0 = r[6], u1 = r[7];
    u2[i] = u0 * u0 + u1 * u1;
    x2[i] = x0 * x0 + x1 * x1;
    double* m = Mx + 8 * i;
    m[0] = -x1 * u0; m[1] = -x1 * u1; m[2] = -x1; m[3] = x0 * u0; m[4] = x0 * u1; m[5] = x0; m[6] = -x1 * u2[i]; m[7] = x0 * u2[i];
  }
  double V1[64], S1[8];
  right_singular_vectors<6, 8>(Mx, V1, S1);
#define V1E(r, c) V1[(r) * 8 + (c)]
  const double a = -V1E(2, 6) * V1E(7, 6) + V1E(5, 6) * V1E(6, 6);
  const double b = ((-V1E(2, 6) * V1E(7, 7) - V1E(2, 7) * V1E(7, 6)) + V1E(5, 6) * V1E(6, 7)) + V1E(5, 7) * V1E(6, 6);
  const double c = -V1E(2, 7) * V1E(7, 7) + V1E(5, 7) * V1E(6, 7);
  const double dd = b * b - 4.0 * a * c;
  int nsols = 0;
  double rs[2] = {0.0, 0.0};
  if ((dd < 100.0 * DBL_EPSILON) && (-dd < 100.0 * DBL_EPSILON)) { nsols = 1; rs[0] = (-b) / (2.0 * a); }
  else if (dd > 0.0) { nsols = 2; const double d2 = sqrt(dd); rs[0] = (-b + d2) / (2.0 * a); rs[1] = (-b - d2) / (2.0 * a); }
  else return 0;
  int nres = 0;
  for (int s = 0; s < nsols; ++s) {
    double n[8];
    for (int k = 0; k < 8; ++k) n[k] = rs[s] * V1E(k, 6) + V1E(k, 7);
    const double l2 = n[6] / n[2];
    if (l2 < lmin || l2 > lmax || !(l2 == l2)) continue;
    double T[30];
    for (int i = 0; i < 6; ++i) {
      const double* r = d + kRadHomDatum * i;
      const double x0 = r[4], u0 = r[6], u1 = r[7];
      const double u3 = 1.0 + l2 * u2[i];
      const double rr = (n[0] * u0 + n[1] * u1) + n[2] * u3;
      T[5 * i + 0] = -Mx[8 * i + 3]; T[5 * i + 1] = -Mx[8 * i + 4]; T[5 * i + 2] = -x0 * u3; T[5 * i + 3] = x2[i] * rr; T[5 * i + 4] = rr;
    }
    double V2[25], S2[5];
    right_singular_vectors<6, 5>(T, V2, S2);
    const double v4 = V2[4 * 5 + 4];
    const double v[4] = {V2[0 * 5 + 4] / v4, V2[1 * 5 + 4] / v4, V2[2 * 5 + 4] / v4, V2[3 * 5 + 4] / v4};
    const double l1 = v[3];
    if (l1 < lmin || l1 > lmax || !(l1 == l1)) continue;
    double* m = models + (size_t)stride * nres;
    for (int k = 0; k < stride; ++k) m[k] = 0.0;
    for (int k = 0; k < 6; ++k) m[k] = n[k];
    m[6] = v[0]; m[7] = v[1]; m[8] = v[2];
    m[9] = l1; m[10] = l2;
    inverse3_cofactor(m, m + 11);
    nres++;
  }
#undef V1E
  return nres;
}

// division-model helpers of six_point_radial_distortion_homography.cc:151-193
RDEV void radhom_distort(const double* p3, double f, double l, double* out) {
  const double px = f * p3[0] / p3[2], py = f * p3[1] / p3[2];
  const double r_u_sq = px * px + py * py;
  const double denom = 2.0 * l * r_u_sq;
  const double inner = 1.0 - 4.0 * l * r_u_sq;
  if (fabs(denom) < DBL_EPSILON || inner < 0.0) { out[0] = px; out[1] = py; }
  else { const double scale = (1.0 - sqrt(inner)) / denom; out[0] = px * scale; out[1] = py * scale; }
}
RDEV void radhom_undistort(const double* p2, double f, double l, double* out3) {
  const double r_d_sq = p2[0] * p2[0] + p2[1] * p2[1];
  const double und = 1.0 / (1.0 + l * r_d_sq);
  out3[0] = p2[0] * und / f; out3[1] = p2[1] * und / f; out3[2] = 1.0;
}
// CheckRadialSymmetricError (:201-239) with the model row {H | l1 | l2 | H^-1}
RDEV double radial_homography_error(const double* m, const double* d) {
  const double f1 = d[8], f2 = d[9];
  const double l1s = m[9] / (f1 * f1), l2s = m[10] / (f2 * f2);
  double bl[3], br[3], y[3], z[3], pl[2], pr[2];
  radhom_undistort(d, f1, l1s, bl);
  radhom_undistort(d + 2, f2, l2s, br);
  for (int i = 0; i < 3; ++i) {
    y[i] = (m[3 * i] * br[0] + m[3 * i + 1] * br[1]) + m[3 * i + 2] * br[2];                   // ray 2 in camera 1
    z[i] = (m[11 + 3 * i] * bl[0] + m[11 + 3 * i + 1] * bl[1]) + m[11 + 3 * i + 2] * bl[2];    // ray 1 in camera 2
  }
  const double yz = y[2], zz = z[2];
  for (int i = 0; i < 3; ++i) { y[i] /= yz; z[i] /= zz; }
  radhom_distort(y, f1, l1s, pl);
  radhom_distort(z, f2, l2s, pr);
  const double dlx = d[0] - pl[0], dly = d[1] - pl[1], drx = d[2] - pr[0], dry = d[3] - pr[1];
  return 0.5 * ((dlx * dlx + dly * dly) + (drx * drx + dry * dry));
}

}  // namespace rsc
}  // namespace thip
