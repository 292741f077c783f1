// five_point_device.h -- the five-point essential-matrix solver on the device (gfx950, FP64), one thread per problem.
// Built with -ffp-contract=off: the operation order below is kept identical to
// the CPU oracle's transcription of the same algorithms, which is what makes
// RANSAC inlier sets bit-identical between the two (DESIGN.md "RANSAC parity").
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>

#include "small_linalg.h"   // FullPivLU, fullpiv_lu, dswap
#include "eig_general.h"    // eig_real_general

namespace thip {
namespace rsc {

// ------------------------------------------------------------ five point
RDEV void mul_deg1(const double* a, const double* b, double* o) {  // five_point_relative_pose.cc:68-92
  o[0] = a[0] * b[0];
  o[1] = a[0] * b[1] + a[1] * b[0];
  o[2] = a[1] * b[1];
  o[3] = a[0] * b[2] + a[2] * b[0];
  o[4] = a[1] * b[2] + a[2] * b[1];
  o[5] = a[2] * b[2];
  o[6] = a[0] * b[3] + a[3] * b[0];
  o[7] = a[1] * b[3] + a[3] * b[1];
  o[8] = a[2] * b[3] + a[3] * b[2];
  o[9] = a[3] * b[3];
}
RDEV void mul_deg2_deg1(const double* a, const double* b, double* o) {  // :96-140
  o[0] = a[0] * b[0];
  o[1] = a[0] * b[1] + a[1] * b[0];
  o[2] = a[1] * b[1] + a[2] * b[0];
  o[3] = a[2] * b[1];
  o[4] = a[0] * b[2] + a[3] * b[0];
  o[5] = a[1] * b[2] + a[3] * b[1] + a[4] * b[0];
  o[6] = a[2] * b[2] + a[4] * b[1];
  o[7] = a[3] * b[2] + a[5] * b[0];
  o[8] = a[4] * b[2] + a[5] * b[1];
  o[9] = a[5] * b[2];
  o[10] = a[0] * b[3] + a[6] * b[0];
  o[11] = a[1] * b[3] + a[6] * b[1] + a[7] * b[0];
  o[12] = a[2] * b[3] + a[7] * b[1];
  o[13] = a[3] * b[3] + a[6] * b[2] + a[8] * b[0];
  o[14] = a[4] * b[3] + a[7] * b[2] + a[8] * b[1];
  o[15] = a[5] * b[3] + a[8] * b[2];
  o[16] = a[6] * b[3] + a[9] * b[0];
  o[17] = a[7] * b[3] + a[9] * b[1];
  o[18] = a[8] * b[3] + a[9] * b[2];
  o[19] = a[9] * b[3];
}

// corr: 5 x [x1 y1 x2 y2]; E: up to 10 row-major 3x3.  Returns #solutions.
// Steps 1-3 of the five-point solver: null space N (9 x 4) and the 10 x 10 action matrix M (false: rank deficient)
__device__ __attribute__((noinline)) bool five_point_pre(const double* corr, double* N, double* M) {
  // Step 1: 5x9 epipolar constraint rows (:228-236)
  double A[45];
  for (int i = 0; i < 5; ++i) {
    const double x1 = corr[4 * i], y1 = corr[4 * i + 1], x2 = corr[4 * i + 2], y2 = corr[4 * i + 3];
    double* r = A + 9 * i;
    r[0] = x2 * x1; r[1] = y2 * x1; r[2] = x1; r[3] = x2 * y1; r[4] = y2 * y1; r[5] = y1; r[6] = x2; r[7] = y2; r[8] = 1.0;
  }
  // null space via full-pivot LU (Eigen FullPivLU::kernel, :242-247)
  FullPivLU f;
  fullpiv_lu(A, 5, 9, f);
  const double premult = fabs(f.maxpivot) * (DBL_EPSILON * 5.0);
  int rank = 0;
  for (int i = 0; i < f.nonzero_pivots; ++i) rank += fabs(A[i * 9 + i]) > premult;
  if (9 - rank != 4) return false;
  int cidx[9];
  for (int j = 0; j < 9; ++j) cidx[j] = j;
  for (int k = 0; k < f.size; ++k) dswap(cidx[k], cidx[f.colt[k]]);
  // solve U1 X = U2 (5x5 upper, 4 right-hand sides)
  double X[20];
  for (int c = 0; c < 4; ++c)
    for (int i = 4; i >= 0; --i) {
      double s = A[i * 9 + 5 + c];
      for (int j = i + 1; j < 5; ++j) s -= A[i * 9 + j] * X[j * 4 + c];
      X[i * 4 + c] = s / A[i * 9 + i];
    }
  for (int i = 0; i < 36; ++i) N[i] = 0.0;   // null_space 9 x 4
  for (int i = 0; i < 5; ++i) for (int c = 0; c < 4; ++c) N[cidx[i] * 4 + c] = -X[i * 4 + c];
  for (int c = 0; c < 4; ++c) N[cidx[5 + c] * 4 + c] = 1.0;
  // null_space_matrix[i][j] = row (3*j + i) of N  (:254-257)
  const double* ns[3][3];
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) ns[i][j] = N + 4 * (3 * j + i);
  // Step 2: constraint matrix 10 x 20 (:142-206)
  double C[200];
  {
    double eet[3][3][10];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) {
      double t0[10], t1[10], t2[10];
      mul_deg1(ns[i][0], ns[j][0], t0); mul_deg1(ns[i][1], ns[j][1], t1); mul_deg1(ns[i][2], ns[j][2], t2);
      for (int k = 0; k < 10; ++k) eet[i][j][k] = 2 * ((t0[k] + t1[k]) + t2[k]);
    }
    double trace[10];
    for (int k = 0; k < 10; ++k) trace[k] = (eet[0][0][k] + eet[1][1][k]) + eet[2][2][k];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) {
      double a[20], b[20], c[20], d[20];
      mul_deg2_deg1(eet[i][0], ns[0][j], a); mul_deg2_deg1(eet[i][1], ns[1][j], b);
      mul_deg2_deg1(eet[i][2], ns[2][j], c); mul_deg2_deg1(trace, ns[i][j], d);
      double* row = C + 20 * (3 * i + j);
      for (int k = 0; k < 20; ++k) row[k] = ((a[k] + b[k]) + c[k]) - 0.5 * d[k];
    }
    double p0[10], p1[10], q[10], d0[20], d1[20], d2[20];
    mul_deg1(ns[0][1], ns[1][2], p0); mul_deg1(ns[0][2], ns[1][1], p1);
    for (int k = 0; k < 10; ++k) q[k] = p0[k] - p1[k];
    mul_deg2_deg1(q, ns[2][0], d0);
    mul_deg1(ns[0][2], ns[1][0], p0); mul_deg1(ns[0][0], ns[1][2], p1);
    for (int k = 0; k < 10; ++k) q[k] = p0[k] - p1[k];
    mul_deg2_deg1(q, ns[2][1], d1);
    mul_deg1(ns[0][0], ns[1][1], p0); mul_deg1(ns[0][1], ns[1][0], p1);
    for (int k = 0; k < 10; ++k) q[k] = p0[k] - p1[k];
    mul_deg2_deg1(q, ns[2][2], d2);
    for (int k = 0; k < 20; ++k) C[180 + k] = (d0[k] + d1[k]) + d2[k];
  }
  // Step 3: eliminated = lu(C[:, :10]).solve(C[:, 10:])  (:260-263)
  double L[100], B[100];
  for (int i = 0; i < 10; ++i) for (int j = 0; j < 10; ++j) { L[i * 10 + j] = C[i * 20 + j]; B[i * 10 + j] = C[i * 20 + 10 + j]; }
  FullPivLU g;
  fullpiv_lu(L, 10, 10, g);
  for (int k = 0; k < 10; ++k) if (g.rowt[k] != k) for (int j = 0; j < 10; ++j) dswap(B[k * 10 + j], B[g.rowt[k] * 10 + j]);
  for (int c = 0; c < 10; ++c) {
    for (int i = 0; i < 10; ++i) { double s = B[i * 10 + c]; for (int j = 0; j < i; ++j) s -= L[i * 10 + j] * B[j * 10 + c]; B[i * 10 + c] = s; }
    for (int i = 9; i >= 0; --i) { double s = B[i * 10 + c]; for (int j = i + 1; j < 10; ++j) s -= L[i * 10 + j] * B[j * 10 + c]; B[i * 10 + c] = s / L[i * 10 + i]; }
  }
  int gidx[10];
  for (int j = 0; j < 10; ++j) gidx[j] = j;
  for (int k = 0; k < 10; ++k) dswap(gidx[k], gidx[g.colt[k]]);
  double El[100];  // eliminated matrix: row gidx[i] = B row i
  for (int i = 0; i < 10; ++i) for (int j = 0; j < 10; ++j) El[gidx[i] * 10 + j] = B[i * 10 + j];
  // action matrix (:265-273)
  for (int i = 0; i < 100; ++i) M[i] = 0.0;
  const int src[6] = {0, 1, 2, 4, 5, 7};
  for (int r = 0; r < 6; ++r) for (int j = 0; j < 10; ++j) M[r * 10 + j] = El[src[r] * 10 + j];
  M[6 * 10 + 0] = -1.0; M[7 * 10 + 1] = -1.0; M[8 * 10 + 3] = -1.0; M[9 * 10 + 6] = -1.0;
  return true;
}
// the last four entries of the NORMALISED eigenvector in column i of Vv (10 x 10 row-major): Eigen normalises
RDEV void five_point_v4(const double* Vv, int i, double* v4) {
  double nrm = 0.0;
  for (int k = 0; k < 10; ++k) nrm += Vv[k * 10 + i] * Vv[k * 10 + i];
  nrm = sqrt(nrm);
  for (int k = 0; k < 4; ++k) v4[k] = Vv[(6 + k) * 10 + i] / nrm;
}
// Map<Matrix<9,1>>(ematrix.data()) = null_space * v  (column-major 3x3) -> E row-major
RDEV void five_point_E(const double* N, const double* v4, double* Eo) {
  double e9[9];
  for (int rI = 0; rI < 9; ++rI) e9[rI] = ((N[rI * 4] * v4[0] + N[rI * 4 + 1] * v4[1]) + N[rI * 4 + 2] * v4[2]) + N[rI * 4 + 3] * v4[3];
  for (int c = 0; c < 3; ++c) for (int rr = 0; rr < 3; ++rr) Eo[rr * 3 + c] = e9[c * 3 + rr];
}
RDEV int five_point(const double* corr, double* E) {
  double N[36], M[100];
  if (!five_point_pre(corr, N, M)) return 0;
  double wr[10], wi[10], Vv[100];
  if (!eig_real_general(10, M, wr, wi, Vv)) return 0;
  int ns_out = 0;
  for (int i = 0; i < 10; ++i) {
    if (wi[i] != 0) continue;  // only real solutions (:281-284)
    double v4[4];
    five_point_v4(Vv, i, v4);
    five_point_E(N, v4, E + 9 * ns_out);
    ns_out++;
  }
  return ns_out;
}

}  // namespace rsc
}  // namespace thip
