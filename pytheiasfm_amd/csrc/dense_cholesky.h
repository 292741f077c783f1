// dense_cholesky.h -- launch interface of the dense SPD solve (dense_cholesky.hip, the BA's K3 kernels), and DenseSpd, the
// owner of one system that the global-pose stages factor and solve against.  ba_kernels.h includes this header.
#pragma once
#include "device_util.h"

namespace thip {

// dense SPD solve  A x = b  (lower triangle of row-major A, leading dim lda;
// A is overwritten by its Cholesky factor, b by x).  fail_flag (device) is
// incremented if a pivot is not positive.
size_t dense_cholesky_workspace(int n);  // doubles
void dense_cholesky_solve(int n, double* A, int lda, double* b, double* work, double* fail_flag, hipStream_t st);
// The same kernels factored once and solved many times (rotation_averaging.hip).  dense_cholesky_factor: rows
// n .. n+k-1 of A (k >= 1) hold k right-hand sides and come out forward-substituted (y = L^-1 b); lda >= n + k;
// work = dense_cholesky_workspace(n) doubles and keeps the 64 x 64 block inverses for the solves below.
// dense_cholesky_back_substitute: X = L^-T Y for k vectors (Y [k][ldy] is overwritten).
// dense_cholesky_solve_factored: X = A^-1 B for k vectors (B [k][ldb] overwritten; T: [k][n] scratch).
// skip (device int, optional): every launch of the three returns at once while *skip is non-zero (lud_positions.hip's
// and nonlinear_rotations.hip's device-side stopping tests); the arithmetic is the same with or without it.
void dense_cholesky_factor(int n, int k, double* A, int lda, double* work, double* fail_flag, hipStream_t st,
                           const int* skip = nullptr);
void dense_cholesky_back_substitute(int n, const double* A, int lda, const double* work, int k, double* Y, int ldy,
                                    double* X, int ldx, hipStream_t st, const int* skip = nullptr);
void dense_cholesky_solve_factored(int n, const double* A, int lda, const double* work, int k, double* B, int ldb,
                                   double* T, double* X, int ldx, hipStream_t st, const int* skip = nullptr);

// One dense system on the device: A [(n + k) x lda], lda = n + k, whose rows n .. n + k - 1 are the right-hand sides of
// the factorisation; the workspace; the fail flag.  The vectors X, Y, B, T of the solves are [.][n].
struct DenseSpd {
  int n = 0, k = 0, lda = 0;
  size_t dense = 0;   // doubles of A
  DevBuf<double> a, work, fail;

  // A stage allocates this before anything else of its own: a system that does not fit is what it reports.
  int alloc(int n_, int k_) {
    n = n_; k = k_; lda = n + k; dense = (size_t)(n + k) * lda;
    int rc;
    if ((rc = a.alloc(dense)) || (rc = work.alloc(dense_cholesky_workspace(n))) || (rc = fail.alloc(1))) return rc;
    return 0;
  }
  double* A() { return a.p; }
  double* flag() { return fail.p; }   // for a kernel that reads and resets it on the device
  double* rhs_row(int r) { return a.p + (size_t)(n + r) * lda; }
  // zeroes A; with_flag: the flag too (once, before the first factorisation)
  int clear(hipStream_t st, bool with_flag = false) {
    HIP_TRY(hipMemsetAsync(a.p, 0, sizeof(double) * dense, st));
    if (with_flag) HIP_TRY(hipMemsetAsync(fail.p, 0, sizeof(double), st));
    return 0;
  }
  void factor(int nrhs, hipStream_t st, const int* skip = nullptr) {   // nrhs <= k right-hand-side rows ride along
    dense_cholesky_factor(n, nrhs, a.p, lda, work.p, fail.p, st, skip);
  }
  void back_substitute(int nv, double* Y, int ldy, double* X, hipStream_t st, const int* skip = nullptr) {
    dense_cholesky_back_substitute(n, a.p, lda, work.p, nv, Y, ldy, X, n, st, skip);
  }
  void solve_factored(int nv, double* B, double* T, double* X, hipStream_t st, const int* skip = nullptr) {
    dense_cholesky_solve_factored(n, a.p, lda, work.p, nv, B, n, T, X, n, st, skip);
  }
  int failed(bool* out) {   // the launches so far, then a blocking read of the flag
    double f = 0.0;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(&f, fail.p, sizeof(double), hipMemcpyDeviceToHost));
    *out = f != 0.0;
    return 0;
  }
};

}  // namespace thip
