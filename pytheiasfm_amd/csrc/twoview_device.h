// twoview_device.h -- two-view geometry on the device (gfx950, FP64), one thread per problem: cheirality and Sampson
// error, the eight-point fundamental matrix, the four-point homography, the pose from an essential matrix, two-view
// triangulation, focal lengths from a fundamental matrix and the uncalibrated relative pose.
// Built with -ffp-contract=off: the operation order below is kept identical to
// the CPU oracle's transcription of the same algorithms, which is what makes
// RANSAC inlier sets bit-identical between the two (DESIGN.md "RANSAC parity").
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>

#include "small_linalg.h"   // FullPivLU, fullpiv_lu, dswap, svd3, det3, svd_sq, matmul3, inverse3

namespace thip {
namespace rsc {

// triangulation.cc:216-232
RDEV bool in_front(const double* c, const double* R, const double* pos) {
  const double d1[3] = {c[0], c[1], 1.0};
  const double h2[3] = {c[2], c[3], 1.0};
  const double d2[3] = {(R[0] * h2[0] + R[3] * h2[1]) + R[6] * h2[2], (R[1] * h2[0] + R[4] * h2[1]) + R[7] * h2[2],
                        (R[2] * h2[0] + R[5] * h2[1]) + R[8] * h2[2]};
  const double d1sq = (d1[0] * d1[0] + d1[1] * d1[1]) + d1[2] * d1[2];
  const double d2sq = (d2[0] * d2[0] + d2[1] * d2[1]) + d2[2] * d2[2];
  const double d1d2 = (d1[0] * d2[0] + d1[1] * d2[1]) + d1[2] * d2[2];
  const double d1p = (d1[0] * pos[0] + d1[1] * pos[1]) + d1[2] * pos[2];
  const double d2p = (d2[0] * pos[0] + d2[1] * pos[1]) + d2[2] * pos[2];
  return (d2sq * d1p - d1d2 * d2p > 0) && (d1d2 * d1p - d1sq * d2p > 0);
}

// pose/util.cc:56-68, y^T F x with x = feature1, y = feature2
RDEV double sampson(const double* F, const double* c) {
  const double x0 = c[0], x1 = c[1], y0 = c[2], y1 = c[3];
  const double ex0 = (F[0] * x0 + F[1] * x1) + F[2];
  const double ex1 = (F[3] * x0 + F[4] * x1) + F[5];
  const double ex2 = (F[6] * x0 + F[7] * x1) + F[8];
  const double num = (y0 * ex0 + y1 * ex1) + ex2;
  const double dn0 = (y0 * F[0] + y1 * F[3]) + F[6];
  const double dn1 = (y0 * F[1] + y1 * F[4]) + F[7];
  const double den = ((dn0 * dn0 + dn1 * dn1) + ex0 * ex0) + ex1 * ex1;
  return num * num / den;
}

// The same error as numerator and denominator (r = a / den): the scoring kernel decides r < thresh without the FP64 division
// whenever a is clear of thresh * den by more than the roundings involved, and divides only at the boundary or when the value
// itself is needed (MLE score of an inlier) -- the decisions and sums are those of the divided form, bit for bit.
RDEV void sampson_parts(const double* F, const double* c, double* a, double* den_out) {
  const double x0 = c[0], x1 = c[1], y0 = c[2], y1 = c[3];
  const double ex0 = (F[0] * x0 + F[1] * x1) + F[2];
  const double ex1 = (F[3] * x0 + F[4] * x1) + F[5];
  const double ex2 = (F[6] * x0 + F[7] * x1) + F[8];
  const double num = (y0 * ex0 + y1 * ex1) + ex2;
  const double dn0 = (y0 * F[0] + y1 * F[3]) + F[6];
  const double dn1 = (y0 * F[1] + y1 * F[4]) + F[7];
  *den_out = ((dn0 * dn0 + dn1 * dn1) + ex0 * ex0) + ex1 * ex1;
  *a = num * num;
}
// fl(a / den) < thresh ?  *r receives the quotient when it had to be (or was asked to be) computed, else stays untouched.
// |fl(t den) - t den| <= eps t den and |fl(a / den) - a / den| <= eps a / den (eps = 2^-53): a margin of 2^-50 covers both.
RDEV bool quotient_below(double a, double den, double thresh, bool want_value, double* r) {
  const double td = thresh * den;
  const double lo = td * (1.0 - 0x1p-50), hi = td * (1.0 + 0x1p-50);
  if (!want_value && a > hi) return false;
  if (!want_value && a < lo) return true;
  if (a > hi) return false;          // an outlier's value is never used
  *r = a / den;
  return *r < thresh;
}

// ---------------------------------------------------------------------------
// Uncalibrated two-view models (plane and known-orientation position: position_plane_device.h)
// ---------------------------------------------------------------------------
// NormalizeImagePoints (sfm/pose/util.cc:81-112): centroid to the origin, RMS
// distance sqrt(2).  pts: n points, `stride` doubles apart; T row-major 3x3.
RDEV void normalize_image_points(const double* pts, int stride, int n, double* out, double* T) {
  double cx = 0.0, cy = 0.0;
  for (int i = 0; i < n; ++i) { cx += pts[i * stride]; cy += pts[i * stride + 1]; }
  cx /= n; cy /= n;
  double ss = 0.0;
  for (int i = 0; i < n; ++i) {
    const double dx = pts[i * stride] - cx, dy = pts[i * stride + 1] - cy;
    ss += dx * dx;
    ss += dy * dy;
  }
  const double rms_mean_dist = sqrt(ss / n);
  const double norm_factor = sqrt(2.0) / rms_mean_dist;
  T[0] = norm_factor; T[1] = 0.0; T[2] = -1.0 * norm_factor * cx;
  T[3] = 0.0; T[4] = norm_factor; T[5] = -1.0 * norm_factor * cy;
  T[6] = 0.0; T[7] = 0.0; T[8] = 1.0;
  for (int i = 0; i < n; ++i) {
    const double x = pts[i * stride], y = pts[i * stride + 1];
    const double hx = (T[0] * x + T[1] * y) + T[2];
    const double hy = (T[3] * x + T[4] * y) + T[5];
    const double hz = (T[6] * x + T[7] * y) + T[8];
    out[2 * i] = hx / hz; out[2 * i + 1] = hy / hz;
  }
}

// NormalizedEightPointFundamentalMatrix for exactly 8 correspondences
// (sfm/pose/eight_point_fundamental_matrix.cc:50-112: the minimal case takes
// the kernel of the 8x9 constraint matrix from a full-pivot LU).
// corr: 8 x [x1 y1 x2 y2]; F row-major with x2^T F x1 = 0.
RDEV bool eight_point_fundamental(const double* corr, double* F) {
  double n1[16], n2[16], T1[9], T2[9];
  normalize_image_points(corr, 4, 8, n1, T1);
  normalize_image_points(corr + 2, 4, 8, n2, T2);
  double A[72];
  for (int i = 0; i < 8; ++i) {
    const double x1 = n1[2 * i], y1 = n1[2 * i + 1], x2 = n2[2 * i], y2 = n2[2 * i + 1];
    double* r = A + 9 * i;
    r[0] = x1 * x2; r[1] = y1 * x2; r[2] = x2;
    r[3] = x1 * y2; r[4] = y1 * y2; r[5] = y2;
    r[6] = x1; r[7] = y1; r[8] = 1.0;
  }
  FullPivLU f;
  fullpiv_lu(A, 8, 9, f);
  const double premult = fabs(f.maxpivot) * (DBL_EPSILON * 8.0);
  int rank = 0;
  for (int i = 0; i < f.nonzero_pivots; ++i) rank += fabs(A[i * 9 + i]) > premult;
  if (9 - rank != 1) return false;   // dimensionOfKernel() != 1
  int cidx[9];
  for (int j = 0; j < 9; ++j) cidx[j] = j;
  for (int k = 0; k < f.size; ++k) dswap(cidx[k], cidx[f.colt[k]]);
  double X[8];
  for (int i = 7; i >= 0; --i) {
    double s = A[i * 9 + 8];
    for (int j = i + 1; j < 8; ++j) s -= A[i * 9 + j] * X[j];
    X[i] = s / A[i * 9 + i];
  }
  double v[9];
  for (int i = 0; i < 9; ++i) v[i] = 0.0;
  for (int i = 0; i < 8; ++i) v[cidx[i]] = -X[i];
  v[cidx[8]] = 1.0;
  // rank-2 projection of the (lazily transposed, :96-105) matrix: row-major reading of v
  double U[9], S[3], V[9];
  svd3(v, U, S, V);
  S[2] = 0.0;
  double US[9], Fr[9];
  for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) US[3 * r + k] = U[3 * r + k] * S[k];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) Fr[3 * r + c] = (US[3 * r] * V[3 * c] + US[3 * r + 1] * V[3 * c + 1]) + US[3 * r + 2] * V[3 * c + 2];
  // undo the normalisation: T2^T F T1 (:107-109)
  double T2t[9], tmp[9];
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) T2t[3 * r + c] = T2[3 * c + r];
  matmul3(T2t, Fr, tmp);
  matmul3(tmp, T1, F);
  return true;
}

// FourPointHomography for exactly 4 correspondences (sfm/pose/four_point_homography.cc:54-105):
// normalised DLT, null vector = last right singular vector of A^T A.
// corr: 4 x [x1 y1 x2 y2]; H row-major with x2 ~ H x1.
// four_point_homography in two pieces around the 9 x 9 SVD (the RANSAC fit runs it by teams of lanes, svd_team.h):
// M = A^T A of the normalised DLT system and the two normalisations, then H = T2^-1 Hn T1 from the last right singular vector
RDEV void four_point_homography_pre(const double* corr, double* M, double* T1, double* T2) {
  double n1[8], n2[8];
  normalize_image_points(corr, 4, 4, n1, T1);
  normalize_image_points(corr + 2, 4, 4, n2, T2);
  double A[72];
  for (int i = 0; i < 4; ++i) {
    const double x1 = n1[2 * i], y1 = n1[2 * i + 1], x2 = n2[2 * i], y2 = n2[2 * i + 1];
    double* r = A + 18 * i;
    r[0] = 0.0; r[1] = 0.0; r[2] = 0.0; r[3] = -x1; r[4] = -y1; r[5] = -1.0; r[6] = x1 * y2; r[7] = y1 * y2; r[8] = y2;
    r[9] = x1; r[10] = y1; r[11] = 1.0; r[12] = 0.0; r[13] = 0.0; r[14] = 0.0; r[15] = -x1 * x2; r[16] = -y1 * x2; r[17] = -x2;
  }
  for (int a = 0; a < 9; ++a)
    for (int b = 0; b < 9; ++b) {
      double s = 0.0;
      for (int k = 0; k < 8; ++k) s += A[9 * k + a] * A[9 * k + b];
      M[9 * a + b] = s;
    }
}
RDEV void four_point_homography_post(const double* Hn, const double* T1, const double* T2, double* H) {
  double T2i[9], tmp[9];
  inverse3(T2, T2i);
  matmul3(T2i, Hn, tmp);
  matmul3(tmp, T1, H);
}

RDEV bool four_point_homography(const double* corr, double* H) {
  double n1[8], n2[8], T1[9], T2[9];
  normalize_image_points(corr, 4, 4, n1, T1);
  normalize_image_points(corr + 2, 4, 4, n2, T2);
  double A[72];
  for (int i = 0; i < 4; ++i) {
    const double x1 = n1[2 * i], y1 = n1[2 * i + 1], x2 = n2[2 * i], y2 = n2[2 * i + 1];
    double* r = A + 18 * i;
    r[0] = 0.0; r[1] = 0.0; r[2] = 0.0; r[3] = -x1; r[4] = -y1; r[5] = -1.0; r[6] = x1 * y2; r[7] = y1 * y2; r[8] = y2;
    r[9] = x1; r[10] = y1; r[11] = 1.0; r[12] = 0.0; r[13] = 0.0; r[14] = 0.0; r[15] = -x1 * x2; r[16] = -y1 * x2; r[17] = -x2;
  }
  double M[81];
  for (int a = 0; a < 9; ++a)
    for (int b = 0; b < 9; ++b) {
      double s = 0.0;
      for (int k = 0; k < 8; ++k) s += A[9 * k + a] * A[9 * k + b];
      M[9 * a + b] = s;
    }
  double U[81], S[9], V[81];
  svd_sq<9>(M, U, S, V);
  double Hn[9];
  for (int k = 0; k < 9; ++k) Hn[k] = V[9 * k + 8];
  double T2i[9], tmp[9];
  inverse3(T2, T2i);
  matmul3(T2i, Hn, tmp);
  matmul3(tmp, T1, H);
  return true;
}

// asymmetric transfer error of HomographyEstimator::Error (estimate_homography.cc:106-112)
RDEV double homography_error(const double* H, const double* c) {
  const double x = c[0], y = c[1];
  const double px = (H[0] * x + H[1] * y) + H[2];
  const double py = (H[3] * x + H[4] * y) + H[5];
  const double pz = (H[6] * x + H[7] * y) + H[8];
  const double ex = c[2] - px / pz, ey = c[3] - py / pz;
  return ex * ex + ey * ey;
}

// essential_matrix_utils.cc:57-80,109-149.  Returns #points in front.
RDEV int best_pose_from_E(const double* E, const double* corr, int ncorr, double* Rout, double* posout) {
  double U[9], S[3], V[9];
  svd3(E, U, S, V);
  if (det3(U) < 0) for (int k = 0; k < 3; ++k) U[k * 3 + 2] = -U[k * 3 + 2];
  if (det3(V) < 0) for (int k = 0; k < 3; ++k) V[k * 3 + 2] = -V[k * 3 + 2];
  // R1 = U d V^T, R2 = U d^T V^T, d = [0 1 0; -1 0 0; 0 0 1]
  double Ud[9], Udt[9];
  for (int i = 0; i < 3; ++i) {
    Ud[i * 3 + 0] = -U[i * 3 + 1]; Ud[i * 3 + 1] = U[i * 3 + 0]; Ud[i * 3 + 2] = U[i * 3 + 2];
    Udt[i * 3 + 0] = U[i * 3 + 1]; Udt[i * 3 + 1] = -U[i * 3 + 0]; Udt[i * 3 + 2] = U[i * 3 + 2];
  }
  double R[2][9];
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) {
    R[0][i * 3 + j] = (Ud[i * 3] * V[j * 3] + Ud[i * 3 + 1] * V[j * 3 + 1]) + Ud[i * 3 + 2] * V[j * 3 + 2];
    R[1][i * 3 + j] = (Udt[i * 3] * V[j * 3] + Udt[i * 3 + 1] * V[j * 3 + 1]) + Udt[i * 3 + 2] * V[j * 3 + 2];
  }
  double t[3] = {U[2], U[5], U[8]};
  const double tn = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
  t[0] /= tn; t[1] /= tn; t[2] /= tn;
  int best = -1, bestcount = -1;
  double bestpos[3] = {0, 0, 0};
  for (int k = 0; k < 4; ++k) {
    const double* Rk = R[k >> 1];
    const double sg = (k & 1) ? -1.0 : 1.0;
    const double tk[3] = {sg * t[0], sg * t[1], sg * t[2]};
    // position = -R^T * translation
    const double pos[3] = {-((Rk[0] * tk[0] + Rk[3] * tk[1]) + Rk[6] * tk[2]), -((Rk[1] * tk[0] + Rk[4] * tk[1]) + Rk[7] * tk[2]),
                           -((Rk[2] * tk[0] + Rk[5] * tk[1]) + Rk[8] * tk[2])};
    int cnt = 0;
    for (int i = 0; i < ncorr; ++i) cnt += in_front(corr + 4 * i, Rk, pos) ? 1 : 0;
    if (cnt > bestcount) { bestcount = cnt; best = k; bestpos[0] = pos[0]; bestpos[1] = pos[1]; bestpos[2] = pos[2]; }
  }
  for (int i = 0; i < 9; ++i) Rout[i] = R[best >> 1][i];
  posout[0] = bestpos[0]; posout[1] = bestpos[1]; posout[2] = bestpos[2];
  return bestcount;
}

// ---- EstimateTriangulation (estimate_triangulation.cc:69-101, triangulation.cc:66-125,160-175,
// essential_matrix_utils.cc:86-107).  obs: two PointObservation rows of 33 doubles (layout: theia_hip.h).
// Triangulate(): E from the two projection matrices, Lindstrom's optimal image points, DLT null vector.
RDEV bool triangulate_two_views(const double* obs, double* X) {
  const double* P1 = obs;
  const double* P2 = obs + 33;
  const double x1[2] = {obs[12], obs[13]}, x2[2] = {obs[33 + 12], obs[33 + 13]};
  // relative_rotation = R1 R2^T, translation = (t1 - relative_rotation t2).normalized(), E = [t]x relative_rotation
  double Rr[9], t[3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Rr[3 * i + j] = (P1[4 * i] * P2[4 * j] + P1[4 * i + 1] * P2[4 * j + 1]) + P1[4 * i + 2] * P2[4 * j + 2];
  for (int i = 0; i < 3; ++i) t[i] = P1[4 * i + 3] - ((Rr[3 * i] * P2[3] + Rr[3 * i + 1] * P2[7]) + Rr[3 * i + 2] * P2[11]);
  const double tn = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
  for (int i = 0; i < 3; ++i) t[i] /= tn;
  double E[9];
  for (int j = 0; j < 3; ++j) {
    E[j] = -t[2] * Rr[3 + j] + t[1] * Rr[6 + j];
    E[3 + j] = t[2] * Rr[j] - t[0] * Rr[6 + j];
    E[6 + j] = -t[1] * Rr[j] + t[0] * Rr[3 + j];
  }
  // FindOptimalImagePoints (triangulation.cc:66-103)
  const double p1[3] = {x1[0], x1[1], 1.0}, p2[3] = {x2[0], x2[1], 1.0};
  double l1[2], l2[2];   // epipolar_line1 = S E p2, epipolar_line2 = S E^T p1
  for (int i = 0; i < 2; ++i) {
    l1[i] = (E[3 * i] * p2[0] + E[3 * i + 1] * p2[1]) + E[3 * i + 2] * p2[2];
    l2[i] = (E[i] * p1[0] + E[3 + i] * p1[1]) + E[6 + i] * p1[2];
  }
  const double Et[4] = {E[0], E[1], E[3], E[4]};   // top-left 2 x 2
  const double a = l1[0] * (Et[0] * l2[0] + Et[1] * l2[1]) + l1[1] * (Et[2] * l2[0] + Et[3] * l2[1]);
  const double b = ((l1[0] * l1[0] + l1[1] * l1[1]) + (l2[0] * l2[0] + l2[1] * l2[1])) / 2.0;
  double c = 0.0;
  for (int i = 0; i < 3; ++i) c += p1[i] * ((E[3 * i] * p2[0] + E[3 * i + 1] * p2[1]) + E[3 * i + 2] * p2[2]);
  const double d = sqrt(b * b - a * c);
  double lambda = c / (b + d);
  {
    const double n1[2] = {l1[0] - lambda * (Et[0] * l1[0] + Et[1] * l1[1]), l1[1] - lambda * (Et[2] * l1[0] + Et[3] * l1[1])};
    const double n2[2] = {l2[0] - lambda * (Et[0] * l2[0] + Et[2] * l2[1]), l2[1] - lambda * (Et[1] * l2[0] + Et[3] * l2[1])};
    l1[0] = n1[0]; l1[1] = n1[1]; l2[0] = n2[0]; l2[1] = n2[1];
  }
  lambda *= (2.0 * d) / ((l1[0] * l1[0] + l1[1] * l1[1]) + (l2[0] * l2[0] + l2[1] * l2[1]));
  const double c1[2] = {p1[0] - lambda * l1[0], p1[1] - lambda * l1[1]};   // hnormalized(): the third coordinate stays 1
  const double c2[2] = {p2[0] - lambda * l2[0], p2[1] - lambda * l2[1]};
  // TriangulateDLT (triangulation.cc:160-175): last right singular vector of the 4 x 4 design matrix
  double A[16], U[16], S[4], V[16];
  for (int j = 0; j < 4; ++j) {
    A[j] = c1[0] * P1[8 + j] - P1[j];
    A[4 + j] = c1[1] * P1[8 + j] - P1[4 + j];
    A[8 + j] = c2[0] * P2[8 + j] - P2[j];
    A[12 + j] = c2[1] * P2[8 + j] - P2[4 + j];
  }
  svd_sq<4>(A, U, S, V);
  for (int i = 0; i < 4; ++i) X[i] = V[4 * i + 3];
  // IsPointInFrontOfCamera for both (estimate_triangulation.cc:62-66,82-87)
  const double z1 = ((X[0] * P1[8] + X[1] * P1[9]) + X[2] * P1[10]) + X[3] * P1[11];
  const double z2 = ((X[0] * P2[8] + X[1] * P2[9]) + X[2] * P2[10]) + X[3] * P2[11];
  return z1 > 0.0 && z2 > 0.0;
}

// FocalLengthsFromFundamentalMatrix (sfm/pose/fundamental_matrix_util.cc:57-130).
// F row-major.  Epipoles = last right singular vectors of F and F^T.
RDEV bool focal_lengths_from_fundamental(const double* F, double* f1, double* f2) {
  double U[9], S[3], V[9], Ft[9];
  svd3(F, U, S, V);
  const double e1[3] = {V[2], V[5], V[8]};
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) Ft[3 * r + c] = F[3 * c + r];
  svd3(Ft, U, S, V);
  const double e2[3] = {V[2], V[5], V[8]};
  if (e1[0] == 0 || e2[0] == 0) return false;
  const double theta1 = atan2(-e1[1], e1[0]);
  const double theta2 = atan2(-e2[1], e2[0]);
  const double R1[9] = {cos(theta1), -sin(theta1), 0.0, sin(theta1), cos(theta1), 0.0, 0.0, 0.0, 1.0};
  const double R2[9] = {cos(theta2), -sin(theta2), 0.0, sin(theta2), cos(theta2), 0.0, 0.0, 0.0, 1.0};
  double R1t[9], tmp[9], rotF[9];
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R1t[3 * r + c] = R1[3 * c + r];
  matmul3(R2, F, tmp);
  matmul3(tmp, R1t, rotF);
  double re1[3], re2[3];
  for (int r = 0; r < 3; ++r) {
    re1[r] = (R1[3 * r] * e1[0] + R1[3 * r + 1] * e1[1]) + R1[3 * r + 2] * e1[2];
    re2[r] = (R2[3 * r] * e2[0] + R2[3 * r + 1] * e2[1]) + R2[3 * r + 2] * e2[2];
  }
  const double d2i[3] = {1.0 / re2[2], 1.0, 1.0 / (-re2[0])};
  const double d1i[3] = {1.0 / re1[2], 1.0, 1.0 / (-re1[0])};
  const double a = (d2i[0] * rotF[0]) * d1i[0];
  const double b = (d2i[0] * rotF[1]) * d1i[1];
  const double c = (d2i[1] * rotF[3]) * d1i[0];
  const double d = (d2i[1] * rotF[4]) * d1i[1];
  const double f1sq = (-a * c * re1[0] * re1[0]) / (a * c * re1[2] * re1[2] + b * d);
  const double f2sq = (-a * b * re2[0] * re2[0]) / (a * b * re2[2] * re2[2] + c * d);
  if (f1sq < 0 || f2sq < 0) return false;
  *f1 = sqrt(f1sq);
  *f2 = sqrt(f2sq);
  return true;
}

// UncalibratedRelativePoseEstimator::EstimateModel (estimate_uncalibrated_relative_pose.cc:83-138).
// corr: 8 x [x1 y1 x2 y2], principal point removed; minmax = {min, max} focal length or null.
// model: F(9) R(9) position(3) focal_length1 focal_length2
RDEV bool uncalibrated_relative_pose(const double* corr, const double* minmax, double* model) {
  double* F = model;
  if (!eight_point_fundamental(corr, F)) return false;
  double f1, f2;
  if (!focal_lengths_from_fundamental(F, &f1, &f2)) return false;
  if (minmax && minmax[0] >= 1.0 && minmax[1] >= 1.0) {
    if (f1 < minmax[0] || f2 < minmax[0] || f1 > minmax[1] || f2 > minmax[1]) return false;
  }
  // EssentialMatrixFromFundamentalMatrix (fundamental_matrix_util.cc:239-249): diag(f2,f2,1) F diag(f1,f1,1)
  const double dl[3] = {f2, f2, 1.0}, dr[3] = {f1, f1, 1.0};
  double E[9];
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) E[3 * r + c] = (dl[r] * F[3 * r + c]) * dr[c];
  double nc[32];
  for (int i = 0; i < 8; ++i) {
    nc[4 * i] = corr[4 * i] / f1; nc[4 * i + 1] = corr[4 * i + 1] / f1;
    nc[4 * i + 2] = corr[4 * i + 2] / f2; nc[4 * i + 3] = corr[4 * i + 3] / f2;
  }
  best_pose_from_E(E, nc, 8, model + 9, model + 18);
  model[21] = f1; model[22] = f2;
  return true;
}

// UncalibratedRelativePoseEstimator::Error (:181-196): cheirality on the focal-normalised
// correspondence, then the Sampson distance under F in (centred) pixels
RDEV double uncalibrated_relative_pose_error(const double* m, const double* d) {
  const double nd[4] = {d[0] / m[21], d[1] / m[21], d[2] / m[22], d[3] / m[22]};
  if (!in_front(nd, m + 9, m + 18)) return DBL_MAX;
  return sampson(m, d);
}

}  // namespace rsc
}  // namespace thip
