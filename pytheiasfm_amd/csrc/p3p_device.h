// p3p_device.h -- Kneip's perspective-three-point solver on the device (gfx950, FP64), one thread per problem.
// Built with -ffp-contract=off: the operation order below is kept identical to
// the CPU oracle's transcription of the same algorithms, which is what makes
// RANSAC inlier sets bit-identical between the two (DESIGN.md "RANSAC parity").
#pragma once
#include <hip/hip_runtime.h>

#include "small_linalg.h"   // cross3, dot3, normalize3, dswap
#include "eig_general.h"    // poly_roots_real_parts

namespace thip {
namespace rsc {

// ----------------------------------------------------------------- P3P
// perspective_three_point.cc:187-291.  corr: 3 x [u v X Y Z].
// R: up to 4 row-major 3x3 (world -> camera), t: up to 4 translations.
RDEV int p3p(const double* corr, double* Rs, double* ts) {
  double f[3][3], wp[3][3];
  for (int i = 0; i < 3; ++i) {
    f[i][0] = corr[5 * i]; f[i][1] = corr[5 * i + 1]; f[i][2] = 1.0;
    normalize3(f[i]);
    wp[i][0] = corr[5 * i + 2]; wp[i][1] = corr[5 * i + 3]; wp[i][2] = corr[5 * i + 4];
  }
  double w10[3], w20[3], cr[3];
  for (int k = 0; k < 3; ++k) { w10[k] = wp[1][k] - wp[0][k]; w20[k] = wp[2][k] - wp[0][k]; }
  cross3(w10, w20, cr);
  if (dot3(cr, cr) < 1e-6) return 0;
  double T[9];  // intermediate camera frame, rows
  auto build_T = [&]() {
    for (int k = 0; k < 3; ++k) T[k] = f[0][k];
    cross3(f[0], f[1], T + 6); normalize3(T + 6);
    cross3(T + 6, T, T + 3);
  };
  build_T();
  double ip[3] = {dot3(T, f[2]), dot3(T + 3, f[2]), dot3(T + 6, f[2])};
  if (ip[2] > 0) {
    for (int k = 0; k < 3; ++k) { dswap(f[0][k], f[1][k]); }
    build_T();
    ip[0] = dot3(T, f[2]); ip[1] = dot3(T + 3, f[2]); ip[2] = dot3(T + 6, f[2]);
    for (int k = 0; k < 3; ++k) dswap(wp[0][k], wp[1][k]);
    for (int k = 0; k < 3; ++k) { w10[k] = wp[1][k] - wp[0][k]; w20[k] = wp[2][k] - wp[0][k]; }
  }
  double Nw[9];  // intermediate world frame, rows
  for (int k = 0; k < 3; ++k) Nw[k] = w10[k];
  normalize3(Nw);
  cross3(Nw, w20, Nw + 6); normalize3(Nw + 6);
  cross3(Nw + 6, Nw, Nw + 3);
  const double iw[3] = {dot3(Nw, w20), dot3(Nw + 3, w20), dot3(Nw + 6, w20)};
  const double d_12 = sqrt(dot3(w10, w10));
  // SolvePlaneRotation (:56-137)
  const double f_1 = ip[0] / ip[2], f_2 = ip[1] / ip[2];
  const double p_1 = iw[0], p_2 = iw[1];
  const double cos_beta = dot3(f[0], f[1]);
  double b = 1.0 / (1.0 - cos_beta * cos_beta) - 1.0;
  b = (cos_beta < 0) ? -sqrt(b) : sqrt(b);
  const double f_1_pw2 = f_1 * f_1, f_2_pw2 = f_2 * f_2;
  const double p_1_pw2 = p_1 * p_1, p_1_pw3 = p_1_pw2 * p_1, p_1_pw4 = p_1_pw3 * p_1;
  const double p_2_pw2 = p_2 * p_2, p_2_pw3 = p_2_pw2 * p_2, p_2_pw4 = p_2_pw3 * p_2;
  const double d_12_pw2 = d_12 * d_12, b_pw2 = b * b;
  double co[5];
  co[0] = -f_2_pw2 * p_2_pw4 - p_2_pw4 * f_1_pw2 - p_2_pw4;
  co[1] = 2.0 * p_2_pw3 * d_12 * b + 2.0 * f_2_pw2 * p_2_pw3 * d_12 * b - 2.0 * f_2 * p_2_pw3 * f_1 * d_12;
  co[2] = -f_2_pw2 * p_2_pw2 * p_1_pw2 - f_2_pw2 * p_2_pw2 * d_12_pw2 * b_pw2 - f_2_pw2 * p_2_pw2 * d_12_pw2 +
          f_2_pw2 * p_2_pw4 + p_2_pw4 * f_1_pw2 + 2.0 * p_1 * p_2_pw2 * d_12 +
          2.0 * f_1 * f_2 * p_1 * p_2_pw2 * d_12 * b - p_2_pw2 * p_1_pw2 * f_1_pw2 +
          2.0 * p_1 * p_2_pw2 * f_2_pw2 * d_12 - p_2_pw2 * d_12_pw2 * b_pw2 - 2.0 * p_1_pw2 * p_2_pw2;
  co[3] = 2.0 * p_1_pw2 * p_2 * d_12 * b + 2.0 * f_2 * p_2_pw3 * f_1 * d_12 - 2.0 * f_2_pw2 * p_2_pw3 * d_12 * b -
          2.0 * p_1 * p_2 * d_12_pw2 * b;
  co[4] = -2 * f_2 * p_2_pw2 * f_1 * p_1 * d_12 * b + f_2_pw2 * p_2_pw2 * d_12_pw2 + 2.0 * p_1_pw3 * d_12 -
          p_1_pw2 * d_12_pw2 + f_2_pw2 * p_2_pw2 * p_1_pw2 - p_1_pw4 - 2.0 * f_2_pw2 * p_2_pw2 * p_1 * d_12 +
          p_2_pw2 * f_1_pw2 * p_1_pw2 + f_2_pw2 * p_2_pw2 * d_12_pw2 * b_pw2;
  double roots[4];
  const int nroots = poly_roots_real_parts(co, 5, roots);
  for (int i = 0; i < nroots; ++i) {
    const double cos_theta = roots[i];
    const double cot_alpha = (-f_1 * p_1 / f_2 - cos_theta * p_2 + d_12 * b) / (-f_1 * cos_theta * p_2 / f_2 + p_1 - d_12);
    // Backsubstitute (:142-183)
    const double sin_theta = sqrt(1.0 - cos_theta * cos_theta);
    const double sin_alpha = sqrt(1.0 / (cot_alpha * cot_alpha + 1.0));
    double cos_alpha = sqrt(1.0 - sin_alpha * sin_alpha);
    if (cot_alpha < 0) cos_alpha = -cos_alpha;
    const double c_nu[3] = {d_12 * cos_alpha * (sin_alpha * b + cos_alpha),
                            cos_theta * d_12 * sin_alpha * (sin_alpha * b + cos_alpha),
                            sin_theta * d_12 * sin_alpha * (sin_alpha * b + cos_alpha)};
    double tr[3];
    for (int k = 0; k < 3; ++k) tr[k] = wp[0][k] + ((Nw[k] * c_nu[0] + Nw[3 + k] * c_nu[1]) + Nw[6 + k] * c_nu[2]);
    const double Q[9] = {-cos_alpha, -sin_alpha * cos_theta, -sin_alpha * sin_theta,
                         sin_alpha, -cos_alpha * cos_theta, -cos_alpha * sin_theta,
                         0, -sin_theta, cos_theta};
    // rotation = (N^T Q^T T)^T = T^T Q N
    double QN[9];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) QN[r * 3 + c] = (Q[r * 3] * Nw[c] + Q[r * 3 + 1] * Nw[3 + c]) + Q[r * 3 + 2] * Nw[6 + c];
    double* R = Rs + 9 * i;
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R[r * 3 + c] = (T[r] * QN[c] + T[3 + r] * QN[3 + c]) + T[6 + r] * QN[6 + c];
    double* t = ts + 3 * i;
    for (int r = 0; r < 3; ++r) t[r] = -((R[r * 3] * tr[0] + R[r * 3 + 1] * tr[1]) + R[r * 3 + 2] * tr[2]);
  }
  return nroots;
}

}  // namespace rsc
}  // namespace thip
