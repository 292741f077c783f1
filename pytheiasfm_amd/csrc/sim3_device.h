// sim3_device.h -- Sophus' Sim(3) exponential and logarithm with the exponential's derivatives, host and device, for
// OptimizeAlignmentSim3 (sfm/transformation/align_point_clouds.cc:161-317, alignment_error.h; csrc/sim3_alignment.hip,
// DESIGN.md 3.6v).  Restated operation for operation from libraries/Sophus/sophus: Sim3::exp (sim3.hpp:557-572),
// RxSO3::expAndTheta (rxso3.hpp:600-619), SO3::expAndTheta (so3.hpp:584-620), details::calcW / calcW_derivatives / calcWInv
// (sim_details.hpp), Sim3::log (sim3.hpp:144-164), RxSO3::logAndTheta (rxso3.hpp:175-185), SO3::logAndTheta
// (so3.hpp:247-291), RxSO3::matrix (rxso3.hpp:192-221) and Eigen's quaternion <-> matrix conversions.  Same branch thresholds
// (Constants<double>::epsilon() = 1e-10) and the same branch taken.  Compile without FMA contraction.
//
// TANGENT ORDER: Sophus', a = [upsilon(3), omega(3), sigma] -- translation part first, rotation vector, logarithm of the
// scale.  The reference's comments (alignment_error.h:54, align_point_clouds.cc:195) say [rx, ry, rz, tx, ty, tz, scale]; the
// code they sit on does not.  upsilon is not the translation: t = W(omega, sigma) upsilon.
//
// DERIVATIVES: the reference differentiates with Ceres' Jets, which differentiate the branch that was taken.  In a small-angle
// or small-sigma branch the branch's constants therefore have derivative zero (theta = 0, A = 1/2, B = 1/6, C = 1), which is
// not always the limit of the true derivative (dC/dsigma -> 1/2); sim3_exp_d returns what the Jets return.
#pragma once
#include <cmath>

#ifndef S3D
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define S3D __host__ __device__ inline
#else
#define S3D inline
#endif
#endif

namespace thip {
namespace sim3 {

constexpr double kEps = 1e-10;                    // Constants<double>::epsilon()
constexpr double kEpsPlus = kEps * (1.0 + kEps);  // Constants<double>::epsilonPlus()

// RxSO3::matrix(): the scaled rotation of the non-unit quaternion (w, v); row-major
S3D void rxso3_matrix(double w, const double* v, double* sR) {
  const double vx_sq = v[0] * v[0], vy_sq = v[1] * v[1], vz_sq = v[2] * v[2], w_sq = w * w;
  const double two_vx = 2.0 * v[0], two_vy = 2.0 * v[1], two_vz = 2.0 * v[2];
  const double two_vx_vy = two_vx * v[1], two_vx_vz = two_vx * v[2], two_vx_w = two_vx * w;
  const double two_vy_vz = two_vy * v[2], two_vy_w = two_vy * w, two_vz_w = two_vz * w;
  sR[0] = vx_sq - vy_sq - vz_sq + w_sq;
  sR[3] = two_vx_vy + two_vz_w;
  sR[6] = two_vx_vz - two_vy_w;
  sR[1] = two_vx_vy - two_vz_w;
  sR[4] = -vx_sq + vy_sq - vz_sq + w_sq;
  sR[7] = two_vx_w + two_vy_vz;
  sR[2] = two_vx_vz + two_vy_w;
  sR[5] = -two_vx_w + two_vy_vz;
  sR[8] = -vx_sq - vy_sq + vz_sq + w_sq;
}
// its derivative along (dw, dv)
S3D void rxso3_matrix_d(double w, const double* v, double dw, const double* dv, double* d) {
  const double xx = 2.0 * (v[0] * dv[0]), yy = 2.0 * (v[1] * dv[1]), zz = 2.0 * (v[2] * dv[2]), ww = 2.0 * (w * dw);
  const double xy = 2.0 * (dv[0] * v[1] + v[0] * dv[1]), xz = 2.0 * (dv[0] * v[2] + v[0] * dv[2]);
  const double yz = 2.0 * (dv[1] * v[2] + v[1] * dv[2]);
  const double xw = 2.0 * (dv[0] * w + v[0] * dw), yw = 2.0 * (dv[1] * w + v[1] * dw), zw = 2.0 * (dv[2] * w + v[2] * dw);
  d[0] = xx - yy - zz + ww;
  d[3] = xy + zw;
  d[6] = xz - yw;
  d[1] = xy - zw;
  d[4] = -xx + yy - zz + ww;
  d[7] = xw + yz;
  d[2] = xz + yw;
  d[5] = -xw + yz;
  d[8] = -xx - yy + zz + ww;
}

S3D void hat(const double* o, double* M) {
  M[0] = 0.0;   M[1] = -o[2]; M[2] = o[1];
  M[3] = o[2];  M[4] = 0.0;   M[5] = -o[0];
  M[6] = -o[1]; M[7] = o[0];  M[8] = 0.0;
}
S3D void mul33(const double* A, const double* B, double* C) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) C[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
}
S3D void mul3v(const double* A, const double* x, double* y) {
  for (int r = 0; r < 3; ++r) y[r] = (A[3 * r] * x[0] + A[3 * r + 1] * x[1]) + A[3 * r + 2] * x[2];
}

// Sim3::exp(a), and with D its derivative as the Jets give it.  sR [9] row-major = rxso3().matrix(), t [3];
// dsR [9][7], dt [3][7]: entry e, parameter k at [7 e + k].
template <bool D>
S3D void exp_impl(const double* a, double* sR, double* t, double* dsR, double* dt) {
  const double* upsilon = a;
  const double* omega = a + 3;
  const double sigma = a[6];
  // RxSO3::expAndTheta
  const double scale_raw = exp(sigma);
  double scale = fmax(scale_raw, kEpsPlus);
  scale = fmin(scale, 1.0 / kEpsPlus);
  const bool clamped = scale != scale_raw;
  const double sqrt_scale = sqrt(scale);
  // SO3::expAndTheta
  const double theta_sq = (omega[0] * omega[0] + omega[1] * omega[1]) + omega[2] * omega[2];
  const bool small_rot = theta_sq < kEps * kEps;
  double theta, imag_factor, real_factor, half_theta = 0.0, sin_half = 0.0;
  if (small_rot) {
    theta = 0.0;
    const double theta_po4 = theta_sq * theta_sq;
    imag_factor = 0.5 - (1.0 / 48.0) * theta_sq + (1.0 / 3840.0) * theta_po4;
    real_factor = 1.0 - (1.0 / 8.0) * theta_sq + (1.0 / 384.0) * theta_po4;
  } else {
    theta = sqrt(theta_sq);
    half_theta = 0.5 * theta;
    sin_half = sin(half_theta);
    imag_factor = sin_half / theta;
    real_factor = cos(half_theta);
  }
  const double uw = real_factor;
  const double uv[3] = {imag_factor * omega[0], imag_factor * omega[1], imag_factor * omega[2]};
  const double qw = uw * sqrt_scale;
  const double qv[3] = {uv[0] * sqrt_scale, uv[1] * sqrt_scale, uv[2] * sqrt_scale};
  rxso3_matrix(qw, qv, sR);

  // details::calcW
  double Omega[9], Omega2[9];
  hat(omega, Omega);
  mul33(Omega, Omega, Omega2);
  const double sc = scale_raw;   // calcW takes exp(sigma) without the clamp
  const bool small_sigma = fabs(sigma) < kEps, small_theta = fabs(theta) < kEps;
  double A, B, C, A_ds = 0.0, B_ds = 0.0, C_ds = 0.0, A_dt = 0.0, B_dt = 0.0;
  if (small_sigma) {
    C = 1.0;
    if (small_theta) {
      A = 0.5;
      B = 1.0 / 6.0;
    } else {
      const double th2 = theta * theta, th3 = theta * th2, s = sin(theta), c = cos(theta);
      A = (1.0 - c) / th2;
      B = (theta - s) / (th2 * theta);
      if (D) {
        A_dt = (theta * s + 2.0 * c - 2.0) / th3;
        B_dt = -(2.0 * theta - 3.0 * s + theta * c) / (th3 * theta);
      }
    }
  } else {
    C = (sc - 1.0) / sigma;
    const double sigma_sq = sigma * sigma, sigma_c = sigma * sigma_sq;
    if (D) C_ds = (sc * (sigma - 1.0) + 1.0) / sigma_sq;
    if (small_theta) {
      A = ((sigma - 1.0) * sc + 1.0) / sigma_sq;
      B = (sc * 0.5 * sigma_sq + sc - 1.0 - sigma * sc) / (sigma_sq * sigma);
      if (D) {
        A_ds = (sc * (sigma_sq - 2.0 * sigma + 2.0) - 2.0) / sigma_c;
        B_ds = (sc * (0.5 * sigma_c - (1.0 + 0.5) * sigma_sq + 3.0 * sigma - 3.0) + 3.0) / (sigma_c * sigma);
      }
    } else {
      const double th2 = theta * theta, th3 = theta * th2, s = sin(theta), c0 = cos(theta);
      const double aa = sc * s, bb = sc * c0, cc = th2 + sigma * sigma;
      A = (aa * sigma + (1.0 - bb) * theta) / (theta * cc);
      B = (C - ((bb - 1.0) * sigma + aa * theta) / (cc)) * 1.0 / (th2);
      if (D) {   // calcW_derivatives, the last branch
        const double b_one = bb - 1.0, theta_b_one = theta * b_one, c_sq = cc * cc, theta_sq_c = th2 * cc;
        const double a_theta = theta * aa, b_theta = theta * bb, c_theta = theta * cc, a_sigma = sigma * aa, b_sigma = sigma * bb;
        const double two_sigma = sigma * 2.0, two_theta = theta * 2.0, sigma_b_one = sigma * b_one;
        A_dt = (2.0 * (theta_b_one - a_sigma)) / c_sq + (b_sigma - bb + a_theta + 1.0) / c_theta + (theta_b_one - a_sigma) / theta_sq_c;
        A_ds = (aa - b_theta + a_sigma) / c_theta - (two_sigma * (theta - b_theta + a_sigma)) / (theta * c_sq);
        B_dt = ((two_theta * (b_sigma - sigma + a_theta)) / c_sq - ((aa + b_theta - a_sigma)) / cc) / th2 -
               (2.0 * ((sc - 1.0) / sigma - (b_sigma - sigma + a_theta) / cc)) / th3;
        B_ds = -((b_sigma + a_theta + b_one) / cc + (sc - 1.0) / sigma_sq - (two_sigma * (sigma_b_one + a_theta)) / c_sq - sc / sigma) / th2;
      }
    }
  }
  double W[9];
  for (int k = 0; k < 9; ++k) W[k] = A * Omega[k] + B * Omega2[k];
  W[0] += C; W[4] += C; W[8] += C;
  mul3v(W, upsilon, t);
  if (!D) return;

  // d quaternion: columns omega_k (3 .. 5) and sigma (6); upsilon does not reach it
  for (int e = 0; e < 9; ++e)
    for (int k = 0; k < 3; ++k) dsR[7 * e + k] = 0.0;
  double dtheta[3] = {0.0, 0.0, 0.0};
  for (int k = 0; k < 3; ++k) {
    double dimag, dreal;
    if (small_rot) {
      const double dth2 = 2.0 * omega[k];
      dimag = (-(1.0 / 48.0) + 2.0 * (1.0 / 3840.0) * theta_sq) * dth2;
      dreal = (-(1.0 / 8.0) + 2.0 * (1.0 / 384.0) * theta_sq) * dth2;
    } else {
      dtheta[k] = omega[k] / theta;
      const double dhalf = 0.5 * dtheta[k];
      dimag = (real_factor * dhalf - imag_factor * dtheta[k]) / theta;
      dreal = -(sin_half * dhalf);
    }
    const double dw = dreal * sqrt_scale;
    double dv[3];
    for (int j = 0; j < 3; ++j) dv[j] = (dimag * omega[j] + (j == k ? imag_factor : 0.0)) * sqrt_scale;
    double dm[9];
    rxso3_matrix_d(qw, qv, dw, dv, dm);
    for (int e = 0; e < 9; ++e) dsR[7 * e + 3 + k] = dm[e];
  }
  {
    const double dss = clamped ? 0.0 : scale / (2.0 * sqrt_scale);
    const double dv[3] = {uv[0] * dss, uv[1] * dss, uv[2] * dss};
    double dm[9];
    rxso3_matrix_d(qw, qv, uw * dss, dv, dm);
    for (int e = 0; e < 9; ++e) dsR[7 * e + 6] = dm[e];
  }
  // d t = d(W) upsilon + W d(upsilon)
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 3; ++k) dt[7 * r + k] = W[3 * r + k];
  for (int k = 0; k < 3; ++k) {
    double e[3] = {0.0, 0.0, 0.0}, G[9], GO[9], OG[9], dW[9], col[3];
    e[k] = 1.0;
    hat(e, G);
    mul33(G, Omega, GO);
    mul33(Omega, G, OG);
    const double dA = A_dt * dtheta[k], dB = B_dt * dtheta[k];
    for (int q = 0; q < 9; ++q) dW[q] = (dA * Omega[q] + A * G[q]) + (dB * Omega2[q] + B * (GO[q] + OG[q]));
    mul3v(dW, upsilon, col);
    for (int r = 0; r < 3; ++r) dt[7 * r + 3 + k] = col[r];
  }
  {
    double dW[9], col[3];
    for (int q = 0; q < 9; ++q) dW[q] = A_ds * Omega[q] + B_ds * Omega2[q];
    dW[0] += C_ds; dW[4] += C_ds; dW[8] += C_ds;
    mul3v(dW, upsilon, col);
    for (int r = 0; r < 3; ++r) dt[7 * r + 6] = col[r];
  }
}

S3D void sim3_exp(const double* a, double* sR, double* t) { exp_impl<false>(a, sR, t, nullptr, nullptr); }
S3D void sim3_exp_d(const double* a, double* sR, double* t, double* dsR, double* dt) { exp_impl<true>(a, sR, t, dsR, dt); }

// Eigen::Quaternion(Matrix3): q = (w, x, y, z) of a rotation matrix (row-major)
S3D void quat_from_rot(const double* m, double* w, double* v) {
  double tr = m[0] + m[4] + m[8];
  if (tr > 0.0) {
    tr = sqrt(tr + 1.0);
    *w = 0.5 * tr;
    tr = 0.5 / tr;
    v[0] = (m[7] - m[5]) * tr;
    v[1] = (m[2] - m[6]) * tr;
    v[2] = (m[3] - m[1]) * tr;
  } else {
    int i = 0;
    if (m[4] > m[0]) i = 1;
    if (m[8] > m[4 * i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    tr = sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0);
    v[i] = 0.5 * tr;
    tr = 0.5 / tr;
    *w = (m[3 * k + j] - m[3 * j + k]) * tr;
    v[j] = (m[3 * j + i] + m[3 * i + j]) * tr;
    v[k] = (m[3 * k + i] + m[3 * i + k]) * tr;
  }
}
// Eigen's Quaternion::toRotationMatrix of a unit quaternion
S3D void rot_from_quat(double w, const double* v, double* m) {
  const double tx = 2.0 * v[0], ty = 2.0 * v[1], tz = 2.0 * v[2];
  const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * v[0], txy = ty * v[0], txz = tz * v[0];
  const double tyy = ty * v[1], tyz = tz * v[1], tzz = tz * v[2];
  m[0] = 1.0 - (tyy + tzz); m[1] = txy - twz;         m[2] = txz + twy;
  m[3] = txy + twz;         m[4] = 1.0 - (txx + tzz); m[5] = tyz - twx;
  m[6] = txz - twy;         m[7] = tyz + twx;         m[8] = 1.0 - (txx + tyy);
}

// Sim3(RxSO3(scale, R), t).log().  false where Sophus' SOPHUS_ENSURE would abort (scale outside [1e-10, 1e10), a
// quaternion that cannot be normalised); a is then zero.
S3D bool sim3_log(double scale_in, const double* R, const double* t, double* a) {
  for (int k = 0; k < 7; ++k) a[k] = 0.0;
  if (!(scale_in >= kEps) || !(scale_in < 1.0 / kEps)) return false;
  double qw, qv[3];
  quat_from_rot(R, &qw, qv);
  const double ss = sqrt(scale_in);
  qw *= ss; qv[0] *= ss; qv[1] *= ss; qv[2] *= ss;
  // RxSO3::logAndTheta
  const double scale = ((qv[0] * qv[0] + qv[1] * qv[1]) + qv[2] * qv[2]) + qw * qw;
  const double sigma = log(scale);
  const double length = sqrt(scale);   // SO3(quaternion): normalize()
  if (!(length >= kEps)) return false;
  const double w = qw / length, v[3] = {qv[0] / length, qv[1] / length, qv[2] / length};
  // SO3::logAndTheta
  const double squared_n = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
  double two_atan_nbyw_by_n, theta;
  if (squared_n < kEps * kEps) {
    if (!(fabs(w) >= kEps)) return false;
    const double squared_w = w * w;
    two_atan_nbyw_by_n = 2.0 / w - (2.0 / 3.0) * (squared_n) / (w * squared_w);
    theta = 2.0 * squared_n / w;
  } else {
    const double n = sqrt(squared_n);
    if (fabs(w) < kEps) {
      const double pi = 3.141592653589793238462643383279502884;
      two_atan_nbyw_by_n = w > 0.0 ? pi / n : -pi / n;
    } else {
      two_atan_nbyw_by_n = 2.0 * atan(n / w) / n;
    }
    theta = two_atan_nbyw_by_n * n;
  }
  const double omega[3] = {two_atan_nbyw_by_n * v[0], two_atan_nbyw_by_n * v[1], two_atan_nbyw_by_n * v[2]};
  // details::calcWInv
  double Omega[9], Omega2[9];
  hat(omega, Omega);
  mul33(Omega, Omega, Omega2);
  const double scale_sq = scale * scale, theta_sq = theta * theta, sin_theta = sin(theta), cos_theta = cos(theta);
  double ca, cb, cc;
  if (fabs(sigma * sigma) < kEps) {
    cc = 1.0 - 0.5 * sigma;
    ca = -0.5;
    if (fabs(theta_sq) < kEps) {
      cb = 1.0 / 12.0;
    } else {
      cb = (theta * sin_theta + 2.0 * cos_theta - 2.0) / (2.0 * theta_sq * (cos_theta - 1.0));
    }
  } else {
    const double scale_cu = scale_sq * scale;
    cc = sigma / (scale - 1.0);
    if (fabs(theta_sq) < kEps) {
      ca = (-sigma * scale + scale - 1.0) / ((scale - 1.0) * (scale - 1.0));
      cb = (scale_sq * sigma - 2.0 * scale_sq + scale * sigma + 2.0 * scale) / (2.0 * scale_cu - 6.0 * scale_sq + 6.0 * scale - 2.0);
    } else {
      const double s_sin = scale * sin_theta, s_cos = scale * cos_theta;
      ca = (theta * s_cos - theta - sigma * s_sin) / (theta * (scale_sq - 2.0 * s_cos + 1.0));
      cb = -scale * (theta * s_sin - theta * sin_theta + sigma * s_cos - scale * sigma + sigma * cos_theta - sigma) /
           (theta_sq * (scale_cu - 2.0 * scale * s_cos - scale_sq + 2.0 * s_cos + scale - 1.0));
    }
  }
  double Winv[9];
  for (int k = 0; k < 9; ++k) Winv[k] = ca * Omega[k] + cb * Omega2[k];
  Winv[0] += cc; Winv[4] += cc; Winv[8] += cc;
  mul3v(Winv, t, a);
  a[3] = omega[0]; a[4] = omega[1]; a[5] = omega[2];
  a[6] = sigma;
  return true;
}

// Sim3FromRotationTranslationScale (align_point_clouds.cc:288-298)
S3D bool sim3_from_rts(const double* R, const double* t, double scale, double* a) { return sim3_log(scale, R, t, a); }

// Sim3ToRotationTranslationScale (align_point_clouds.cc:300-317): rotationMatrix() normalises the quaternion, scale() is its
// squared norm.  The quaternion is recomputed here as exp_impl forms it.
S3D void sim3_to_rts(const double* a, double* R, double* t, double* scale) {
  double sR[9];
  sim3_exp(a, sR, t);
  const double* omega = a + 3;
  double sc = exp(a[6]);
  sc = fmax(sc, kEpsPlus);
  sc = fmin(sc, 1.0 / kEpsPlus);
  const double ss = sqrt(sc);
  const double theta_sq = (omega[0] * omega[0] + omega[1] * omega[1]) + omega[2] * omega[2];
  double imag_factor, real_factor;
  if (theta_sq < kEps * kEps) {
    const double theta_po4 = theta_sq * theta_sq;
    imag_factor = 0.5 - (1.0 / 48.0) * theta_sq + (1.0 / 3840.0) * theta_po4;
    real_factor = 1.0 - (1.0 / 8.0) * theta_sq + (1.0 / 384.0) * theta_po4;
  } else {
    const double theta = sqrt(theta_sq), half_theta = 0.5 * theta;
    imag_factor = sin(half_theta) / theta;
    real_factor = cos(half_theta);
  }
  double w = real_factor * ss, v[3] = {imag_factor * omega[0] * ss, imag_factor * omega[1] * ss, imag_factor * omega[2] * ss};
  const double sq = ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + w * w;
  *scale = sq;
  const double n = sqrt(sq);
  w /= n; v[0] /= n; v[1] /= n; v[2] /= n;
  rot_from_quat(w, v, R);
}

// Sim3ToHomogeneousMatrix (transformation_wrapper.cc:125-132): Sim3::exp(a).matrix(), [sR t; 0 0 0 1] row-major
S3D void sim3_to_matrix4(const double* a, double* M) {
  double sR[9], t[3];
  sim3_exp(a, sR, t);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) M[4 * r + c] = sR[3 * r + c];
    M[4 * r + 3] = t[r];
  }
  M[12] = 0.0; M[13] = 0.0; M[14] = 0.0; M[15] = 1.0;
}

}  // namespace sim3
}  // namespace thip
