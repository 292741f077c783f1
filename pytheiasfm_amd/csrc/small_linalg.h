// small_linalg.h -- small dense linear algebra on the device (gfx950, FP64), one thread per matrix: the lowest layer
// under the rotation maps (rotation_maps.h), the eigen-solver (eig_general.h) and the minimal solvers (*_device.h).
//
// The routines restate the published algorithms behind the Eigen calls of the reference:
//   Eigen::FullPivLU   (five_point_relative_pose.cc:242-247,261-263)
//   Eigen::JacobiSVD   (essential_matrix_utils.cc:66-67; 9x9 in sqpnp.cc:234) = two-sided Jacobi
// Built with -ffp-contract=off: the operation order below is kept identical to
// the CPU oracle's transcription of the same algorithms, which is what makes
// RANSAC inlier sets bit-identical between the two (DESIGN.md "RANSAC parity").
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>

// The qualifier of everything in thip::rsc.  Not THIP_DEV (device_util.h): that one is __forceinline__, this is plain
// `inline`, which leaves the large solver bodies to the inliner's own judgement.  Defined here only; every other rsc
// header includes this one, so the order of includes does not matter.
#ifndef RDEV
#define RDEV __device__ inline
#endif

namespace thip {
namespace rsc {

template <typename T>
RDEV void dswap(T& a, T& b) { T t = a; a = b; b = t; }

// ------------------------------------------------------- small linear algebra
// Full-pivot LU of a rows x cols row-major matrix (Eigen::FullPivLU::compute).
// The pivot search scans the remaining corner column by column and keeps the
// first strict maximum.
struct FullPivLU {
  int rows, cols, size, nonzero_pivots;
  double maxpivot;
  int rowt[10], colt[20];
};

RDEV void fullpiv_lu(double* A, int rows, int cols, FullPivLU& f) {
  f.rows = rows; f.cols = cols; f.size = rows < cols ? rows : cols;
  f.nonzero_pivots = f.size; f.maxpivot = 0.0;
  for (int k = 0; k < f.size; ++k) {
    double best = -1.0; int br = k, bc = k;
    for (int j = k; j < cols; ++j)
      for (int i = k; i < rows; ++i) {
        const double a = fabs(A[i * cols + j]);
        if (a > best) { best = a; br = i; bc = j; }
      }
    if (best == 0.0) {
      f.nonzero_pivots = k;
      for (int i = k; i < f.size; ++i) { f.rowt[i] = i; f.colt[i] = i; }
      break;
    }
    if (best > f.maxpivot) f.maxpivot = best;
    f.rowt[k] = br; f.colt[k] = bc;
    if (br != k) for (int j = 0; j < cols; ++j) dswap(A[k * cols + j], A[br * cols + j]);
    if (bc != k) for (int i = 0; i < rows; ++i) dswap(A[i * cols + k], A[i * cols + bc]);
    if (k < rows - 1) for (int i = k + 1; i < rows; ++i) A[i * cols + k] /= A[k * cols + k];
    if (k < f.size - 1)
      for (int i = k + 1; i < rows; ++i)
        for (int j = k + 1; j < cols; ++j) A[i * cols + j] -= A[i * cols + k] * A[k * cols + j];
  }
}

// Two-sided Jacobi SVD of a 3x3 row-major matrix (the algorithm of
// Eigen::JacobiSVD for square real matrices): A = U diag(s) V^T, s sorted
// descending, s >= 0.
RDEV void jacobi_rot_sym(double x, double y, double z, double* c, double* s) {
  // JacobiRotation::makeJacobi for the symmetric 2x2 [[x, y], [y, z]]
  const double deno = 2.0 * fabs(y);
  if (deno < DBL_MIN) { *c = 1.0; *s = 0.0; return; }
  const double tau = (x - z) / deno;
  const double w = sqrt(tau * tau + 1.0);
  const double t = (tau > 0) ? 1.0 / (tau + w) : 1.0 / (tau - w);
  const double sign_t = t > 0 ? 1.0 : -1.0;
  const double n = 1.0 / sqrt(t * t + 1.0);
  *s = -sign_t * (y / fabs(y)) * fabs(t) * n;
  *c = n;
}

// the sweeps, the sign fix and the sort on a work matrix W (destroyed); U, V hold their starting values (identity, or the
// preconditioner's: p4pfr_kernels.hip starts U at a column permutation)
RDEV void svd3_sweeps(double* W, double* U, double* S, double* V) {
  const double precision = 2.0 * DBL_EPSILON;
  double maxdiag = fmax(fabs(W[0]), fmax(fabs(W[4]), fabs(W[8])));
  bool finished = false;
  int sweeps = 0;
  while (!finished && sweeps++ < 64) {
    finished = true;
    for (int p = 1; p < 3; ++p)
      for (int q = 0; q < p; ++q) {
        const double threshold = fmax(DBL_MIN, precision * maxdiag);
        if (fabs(W[p * 3 + q]) > threshold || fabs(W[q * 3 + p]) > threshold) {
          finished = false;
          // real_2x2_jacobi_svd on [[W_pp, W_pq], [W_qp, W_qq]]
          double m00 = W[p * 3 + p], m01 = W[p * 3 + q], m10 = W[q * 3 + p], m11 = W[q * 3 + q];
          double r1c, r1s;
          const double tt = m00 + m11, dd = m10 - m01;
          if (fabs(dd) < DBL_MIN) { r1c = 1.0; r1s = 0.0; }
          else { const double u = tt / dd; const double tmp = sqrt(1.0 + u * u); r1s = 1.0 / tmp; r1c = u / tmp; }
          // m <- rot1 * m  (rows: r0' = c r0 + s r1 ; r1' = -s r0 + c r1)
          const double n00 = r1c * m00 + r1s * m10, n01 = r1c * m01 + r1s * m11;
          const double n11 = -r1s * m01 + r1c * m11;
          double jc, js;
          jacobi_rot_sym(n00, n01, n11, &jc, &js);
          // left rotation L = rot1 * jr^T   (jr = [[jc, js], [-js, jc]])
          const double lc = r1c * jc + r1s * js, ls = r1s * jc - r1c * js;
          // W <- L on rows (p, q): row_p' = lc row_p + ls row_q ; row_q' = -ls row_p + lc row_q
          for (int k = 0; k < 3; ++k) {
            const double a = W[p * 3 + k], b = W[q * 3 + k];
            W[p * 3 + k] = lc * a + ls * b; W[q * 3 + k] = -ls * a + lc * b;
          }
          // U <- U L^T on columns (p, q)
          for (int k = 0; k < 3; ++k) {
            const double a = U[k * 3 + p], b = U[k * 3 + q];
            U[k * 3 + p] = lc * a + ls * b; U[k * 3 + q] = -ls * a + lc * b;
          }
          // W <- W jr on columns (p, q): col_p' = jc col_p - js col_q ; col_q' = js col_p + jc col_q
          for (int k = 0; k < 3; ++k) {
            const double a = W[k * 3 + p], b = W[k * 3 + q];
            W[k * 3 + p] = jc * a - js * b; W[k * 3 + q] = js * a + jc * b;
          }
          for (int k = 0; k < 3; ++k) {
            const double a = V[k * 3 + p], b = V[k * 3 + q];
            V[k * 3 + p] = jc * a - js * b; V[k * 3 + q] = js * a + jc * b;
          }
          maxdiag = fmax(maxdiag, fmax(fabs(W[p * 3 + p]), fabs(W[q * 3 + q])));
        }
      }
  }
  for (int i = 0; i < 3; ++i) {
    const double a = W[i * 3 + i];
    S[i] = fabs(a);
    if (a < 0) for (int k = 0; k < 3; ++k) U[k * 3 + i] = -U[k * 3 + i];
  }
  for (int i = 0; i < 3; ++i) {  // selection sort, descending
    int best = i;
    for (int j = i + 1; j < 3; ++j) if (S[j] > S[best]) best = j;
    if (best != i) {
      dswap(S[i], S[best]);
      for (int k = 0; k < 3; ++k) { dswap(U[k * 3 + i], U[k * 3 + best]); dswap(V[k * 3 + i], V[k * 3 + best]); }
    }
  }
}

RDEV void svd3(const double* Ain, double* U, double* S, double* V) {
  double W[9];
  double scale = 0.0;
  for (int i = 0; i < 9; ++i) scale = fmax(scale, fabs(Ain[i]));
  if (scale == 0.0) scale = 1.0;
  for (int i = 0; i < 9; ++i) W[i] = Ain[i] / scale;
  for (int i = 0; i < 9; ++i) { U[i] = (i % 4 == 0) ? 1.0 : 0.0; V[i] = U[i]; }
  svd3_sweeps(W, U, S, V);
  for (int i = 0; i < 3; ++i) S[i] *= scale;
}

RDEV double det3(const double* M) {
  return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// Two-sided Jacobi SVD of an N x N row-major matrix (Eigen::JacobiSVD for square
// real input: no QR preconditioner), generalisation of svd3 above.
template <int N>
RDEV void svd_sq(const double* Ain, double* U, double* S, double* V) {
  double W[N * N];
  double scale = 0.0;
  for (int i = 0; i < N * N; ++i) scale = fmax(scale, fabs(Ain[i]));
  if (scale == 0.0) scale = 1.0;
  for (int i = 0; i < N * N; ++i) W[i] = Ain[i] / scale;
  for (int i = 0; i < N; ++i) for (int j = 0; j < N; ++j) { U[i * N + j] = (i == j) ? 1.0 : 0.0; V[i * N + j] = U[i * N + j]; }
  const double precision = 2.0 * DBL_EPSILON;
  double maxdiag = 0.0;
  for (int i = 0; i < N; ++i) maxdiag = fmax(maxdiag, fabs(W[i * N + i]));
  bool finished = false;
  int sweeps = 0;
  while (!finished && sweeps++ < 64) {
    finished = true;
    for (int p = 1; p < N; ++p)
      for (int q = 0; q < p; ++q) {
        const double threshold = fmax(DBL_MIN, precision * maxdiag);
        if (fabs(W[p * N + q]) > threshold || fabs(W[q * N + p]) > threshold) {
          finished = false;
          const double m00 = W[p * N + p], m01 = W[p * N + q], m10 = W[q * N + p], m11 = W[q * N + q];
          double r1c, r1s;
          const double tt = m00 + m11, dd = m10 - m01;
          if (fabs(dd) < DBL_MIN) { r1c = 1.0; r1s = 0.0; }
          else { const double u = tt / dd; const double tmp = sqrt(1.0 + u * u); r1s = 1.0 / tmp; r1c = u / tmp; }
          const double n00 = r1c * m00 + r1s * m10, n01 = r1c * m01 + r1s * m11;
          const double n11 = -r1s * m01 + r1c * m11;
          double jc, js;
          jacobi_rot_sym(n00, n01, n11, &jc, &js);
          const double lc = r1c * jc + r1s * js, ls = r1s * jc - r1c * js;
          for (int k = 0; k < N; ++k) {
            const double a = W[p * N + k], b = W[q * N + k];
            W[p * N + k] = lc * a + ls * b; W[q * N + k] = -ls * a + lc * b;
          }
          for (int k = 0; k < N; ++k) {
            const double a = U[k * N + p], b = U[k * N + q];
            U[k * N + p] = lc * a + ls * b; U[k * N + q] = -ls * a + lc * b;
          }
          for (int k = 0; k < N; ++k) {
            const double a = W[k * N + p], b = W[k * N + q];
            W[k * N + p] = jc * a - js * b; W[k * N + q] = js * a + jc * b;
          }
          for (int k = 0; k < N; ++k) {
            const double a = V[k * N + p], b = V[k * N + q];
            V[k * N + p] = jc * a - js * b; V[k * N + q] = js * a + jc * b;
          }
          maxdiag = fmax(maxdiag, fmax(fabs(W[p * N + p]), fabs(W[q * N + q])));
        }
      }
  }
  for (int i = 0; i < N; ++i) {
    const double a = W[i * N + i];
    S[i] = fabs(a);
    if (a < 0) for (int k = 0; k < N; ++k) U[k * N + i] = -U[k * N + i];
  }
  for (int i = 0; i < N; ++i) {  // selection sort, descending
    int best = i;
    for (int j = i + 1; j < N; ++j) if (S[j] > S[best]) best = j;
    if (best != i) {
      dswap(S[i], S[best]);
      for (int k = 0; k < N; ++k) { dswap(U[k * N + i], U[k * N + best]); dswap(V[k * N + i], V[k * N + best]); }
    }
  }
  for (int i = 0; i < N; ++i) S[i] *= scale;
}

// row-major 3x3 product, each entry accumulated left to right
RDEV void matmul3(const double* A, const double* B, double* C) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) C[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
}

// Eigen's 3x3 inverse (Eigen/src/LU/InverseImpl.h compute_inverse<Matrix3d>:
// cofactors of column 0 give the determinant, inverse = cofactor^T / det)
RDEV double cofactor3(const double* m, int i, int j) {
  const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
  return m[3 * i1 + j1] * m[3 * i2 + j2] - m[3 * i1 + j2] * m[3 * i2 + j1];
}
RDEV void inverse3(const double* m, double* inv) {
  const double c00 = cofactor3(m, 0, 0), c10 = cofactor3(m, 1, 0), c20 = cofactor3(m, 2, 0);
  const double det = (c00 * m[0] + c10 * m[3]) + c20 * m[6];
  const double invdet = 1.0 / det;
  inv[0] = c00 * invdet; inv[1] = c10 * invdet; inv[2] = c20 * invdet;
  inv[3] = cofactor3(m, 0, 1) * invdet; inv[4] = cofactor3(m, 1, 1) * invdet; inv[5] = cofactor3(m, 2, 1) * invdet;
  inv[6] = cofactor3(m, 0, 2) * invdet; inv[7] = cofactor3(m, 1, 2) * invdet; inv[8] = cofactor3(m, 2, 2) * invdet;
}

// Eigen's 3 x 3 inverse (Inverse_impl.h compute_inverse_size3_helper): cofactors over the determinant.  Row-major.
RDEV void inverse3_cofactor(const double* m, double* r) {
#define COF(i, j) (m[3 * (((i) + 1) % 3) + (((j) + 1) % 3)] * m[3 * (((i) + 2) % 3) + (((j) + 2) % 3)] - \
                   m[3 * (((i) + 1) % 3) + (((j) + 2) % 3)] * m[3 * (((i) + 2) % 3) + (((j) + 1) % 3)])
  const double c00 = COF(0, 0), c10 = COF(1, 0), c20 = COF(2, 0);
  const double det = (c00 * m[0] + c10 * m[3]) + c20 * m[6];
  const double invdet = 1.0 / det;
  r[0] = c00 * invdet; r[1] = c10 * invdet; r[2] = c20 * invdet;
  r[3] = COF(0, 1) * invdet; r[4] = COF(1, 1) * invdet; r[5] = COF(2, 1) * invdet;
  r[6] = COF(0, 2) * invdet; r[7] = COF(1, 2) * invdet; r[8] = COF(2, 2) * invdet;
#undef COF
}

RDEV void cross3(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
RDEV double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
RDEV void normalize3(double* a) { const double n = sqrt(dot3(a, a)); a[0] /= n; a[1] /= n; a[2] /= n; }

// Eigen::ColPivHouseholderQR of a 4 x 3 system, rank() and solve() (Eigen/src/QR/ColPivHouseholderQR.h:
// computeInPlace, rank with the default threshold eps * diagonalSize, _solve_impl), restated for
// PositionFromTwoRays.  A row-major 4 x 3 (destroyed), b (destroyed).  Returns the rank.
RDEV int colpiv_qr_solve_4x3(double* A, double* b, double* x) {
  const int rows = 4, cols = 3, size = 3;
  double hcoef[3], norm_upd[3], norm_dir[3];
  int transp[3];
  for (int k = 0; k < cols; ++k) {
    double s2 = 0.0;
    for (int r = 0; r < rows; ++r) s2 += A[r * cols + k] * A[r * cols + k];
    norm_upd[k] = norm_dir[k] = sqrt(s2);
  }
  double maxn = fmax(norm_upd[0], fmax(norm_upd[1], norm_upd[2]));
  const double threshold_helper = (maxn * DBL_EPSILON) * (maxn * DBL_EPSILON) / (double)rows;
  const double norm_downdate_threshold = sqrt(DBL_EPSILON);
  int nonzero_pivots = size;
  double maxpivot = 0.0;
  for (int k = 0; k < size; ++k) {
    int big = k;
    for (int j = k + 1; j < cols; ++j) if (norm_upd[j] > norm_upd[big]) big = j;
    const double big_sq = norm_upd[big] * norm_upd[big];
    if (nonzero_pivots == size && big_sq < threshold_helper * (double)(rows - k)) nonzero_pivots = k;
    transp[k] = big;
    if (k != big) {
      for (int r = 0; r < rows; ++r) dswap(A[r * cols + k], A[r * cols + big]);
      dswap(norm_upd[k], norm_upd[big]);
      dswap(norm_dir[k], norm_dir[big]);
    }
    // makeHouseholderInPlace on A(k:, k)
    const double c0 = A[k * cols + k];
    double tail = 0.0;
    for (int r = k + 1; r < rows; ++r) tail += A[r * cols + k] * A[r * cols + k];
    double tau, beta;
    if (tail <= DBL_MIN) {
      tau = 0.0; beta = c0;
      for (int r = k + 1; r < rows; ++r) A[r * cols + k] = 0.0;
    } else {
      beta = sqrt(c0 * c0 + tail);
      if (c0 >= 0.0) beta = -beta;
      for (int r = k + 1; r < rows; ++r) A[r * cols + k] /= (c0 - beta);
      tau = (beta - c0) / beta;
    }
    hcoef[k] = tau;
    A[k * cols + k] = beta;
    if (fabs(beta) > maxpivot) maxpivot = fabs(beta);
    // apply H_k = I - tau v v^T (v = [1; essential]) to the remaining columns
    for (int j = k + 1; j < cols; ++j) {
      double tmp = A[k * cols + j];
      for (int r = k + 1; r < rows; ++r) tmp += A[r * cols + k] * A[r * cols + j];
      A[k * cols + j] -= tau * tmp;
      for (int r = k + 1; r < rows; ++r) A[r * cols + j] -= tau * A[r * cols + k] * tmp;
    }
    for (int j = k + 1; j < cols; ++j) {
      if (norm_upd[j] != 0.0) {
        double temp = fabs(A[k * cols + j]) / norm_upd[j];
        temp = (1.0 + temp) * (1.0 - temp);
        temp = temp < 0.0 ? 0.0 : temp;
        const double q = norm_upd[j] / norm_dir[j];
        const double temp2 = temp * (q * q);
        if (temp2 <= norm_downdate_threshold) {
          double s2 = 0.0;
          for (int r = k + 1; r < rows; ++r) s2 += A[r * cols + j] * A[r * cols + j];
          norm_dir[j] = sqrt(s2);
          norm_upd[j] = norm_dir[j];
        } else {
          norm_upd[j] *= sqrt(temp);
        }
      }
    }
  }
  const double premult = fabs(maxpivot) * (DBL_EPSILON * (double)size);
  int rank = 0;
  for (int i = 0; i < nonzero_pivots; ++i) rank += fabs(A[i * cols + i]) > premult;
  // c = Q^T b, then back-substitution on the leading block, then the column permutation
  for (int k = 0; k < nonzero_pivots; ++k) {
    double tmp = b[k];
    for (int r = k + 1; r < rows; ++r) tmp += A[r * cols + k] * b[r];
    b[k] -= hcoef[k] * tmp;
    for (int r = k + 1; r < rows; ++r) b[r] -= hcoef[k] * A[r * cols + k] * tmp;
  }
  double y[3] = {0.0, 0.0, 0.0};
  for (int i = nonzero_pivots - 1; i >= 0; --i) {
    double s = b[i];
    for (int j = i + 1; j < nonzero_pivots; ++j) s -= A[i * cols + j] * y[j];
    y[i] = s / A[i * cols + i];
  }
  int perm[3] = {0, 1, 2};
  for (int k = 0; k < size; ++k) dswap(perm[k], perm[transp[k]]);
  for (int i = 0; i < 3; ++i) x[i] = 0.0;
  for (int i = 0; i < nonzero_pivots; ++i) x[perm[i]] = y[i];
  return rank;
}

// Right singular vectors by one-sided Jacobi (Hestenes) on the columns of an M x N row-major matrix: V (N x N, row-major),
// columns ordered by decreasing singular value S.  The reference asks Eigen's JacobiSVD for ComputeFullV of a 6 x 8 and a
// 6 x 5 matrix and reads the columns of the smallest singular values; the null space / least-squares direction they span is
// what enters the solver (any basis of the 6 x 8 matrix' null space gives the same homography up to scale).
template <int M, int N>
RDEV void right_singular_vectors(const double* Ain, double* V, double* S) {
  double W[M * N];
  double fro = 0.0;
  for (int i = 0; i < M * N; ++i) { W[i] = Ain[i]; fro += Ain[i] * Ain[i]; }
  for (int i = 0; i < N; ++i) for (int j = 0; j < N; ++j) V[i * N + j] = (i == j) ? 1.0 : 0.0;
  const double tiny2 = (1e-28 * fro > DBL_MIN) ? 1e-28 * fro : DBL_MIN;   // columns below 1e-14 of the matrix norm are null columns
  for (int sweep = 0; sweep < 60; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < N - 1; ++p)
      for (int q = p + 1; q < N; ++q) {
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
        for (int i = 0; i < M; ++i) { const double a = W[i * N + p], b = W[i * N + q]; alpha += a * a; beta += b * b; gamma += a * b; }
        if (alpha < tiny2 || beta < tiny2) continue;
        if (!(fabs(gamma) > 2.0 * DBL_EPSILON * sqrt(alpha * beta))) continue;
        rotated = true;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
        for (int i = 0; i < M; ++i) {
          const double a = W[i * N + p], b = W[i * N + q];
          W[i * N + p] = c * a - s * b; W[i * N + q] = s * a + c * b;
        }
        for (int i = 0; i < N; ++i) {
          const double a = V[i * N + p], b = V[i * N + q];
          V[i * N + p] = c * a - s * b; V[i * N + q] = s * a + c * b;
        }
      }
    if (!rotated) break;
  }
  for (int j = 0; j < N; ++j) { double s2 = 0.0; for (int i = 0; i < M; ++i) s2 += W[i * N + j] * W[i * N + j]; S[j] = sqrt(s2); }
  for (int i = 0; i < N; ++i) {  // selection sort, descending
    int best = i;
    for (int j = i + 1; j < N; ++j) if (S[j] > S[best]) best = j;
    if (best != i) {
      dswap(S[i], S[best]);
      for (int k = 0; k < N; ++k) dswap(V[k * N + i], V[k * N + best]);
    }
  }
}

}  // namespace rsc
}  // namespace thip
