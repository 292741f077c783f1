// dense_cholesky.hip -- K3: dense SPD solve of the reduced camera system on
// gfx950, FP64.  Replaces Ceres' SPARSE_SCHUR + EIGEN_SPARSE SimplicialLDLT of
// the same matrix (bundle_adjustment.h:98,104; selected in bundle_adjuster.cc:63-89).
//
// Blocked right-looking Cholesky on the lower triangle of a row-major matrix.
// The right-hand side is stored as row n of the same (n+1) x lda array, so the
// forward substitution  y = L^-1 b  falls out of the panel solves for free;
// only the backward substitution  x = L^-T y  is separate.
//
// Everything at this size (n = 6 x #cameras ~ 10^3) is LATENCY bound: measured
// on MI355X a dependent FP64 op costs ~22 cycles and sqrt/div several hundred,
// with one wave per SIMD nothing hides it.  Hence:
//   k_potrf : ONE wavefront factors the 64x64 diagonal block in registers
//             (lane = row, pivot row broadcast by v_readlane, 8 partial sums,
//             one rsqrt per column) and also forms its inverse L11^-1;
//   k_trsm  : A21 <- A21 L11^-T as a GEMM with that inverse on the FP64 matrix
//             core (v_mfma_f64_16x16x4_f64): no dependent chains;
//   k_syrk  : trailing update A22 -= L21 L21^T, 64x64 tiles, FP64 MFMA;
//   backward substitution in 64-wide steps with the same block inverses.
#include "ba_kernels.h"
#include "cholesky_device.h"
#include "wave_reduce.h"

#include <algorithm>

namespace thip {
namespace {

using namespace chol;

__global__ __launch_bounds__(256) void k_potrf(double* __restrict__ A, int lda, int k0, int nb,
                                               double* __restrict__ Linv, double* __restrict__ fail_flag,
                                               const int* __restrict__ skip) {
  if (skip && *skip) return;   // workgroup-uniform, before any barrier
  potrf64_wg(A, lda, k0, nb, Linv, fail_flag);
}

// A21 <- A21 * L11^-T for rows [k0 + nb, nrows): X[r][j] = sum_i P[r][i] Z[j][i].
// 128 rows per workgroup; wave w owns rows [32w, 32w + 32).
__global__ __launch_bounds__(256) void k_trsm(double* __restrict__ A, int lda, int nrows, int k0, int nb,
                                              const double* __restrict__ Linv, const int* __restrict__ skip) {
  __shared__ double P[128][LDP];
  __shared__ double Z[NB][LDP];
  if (skip && *skip) return;
  const int tid = threadIdx.x;
  const int r0 = k0 + nb + blockIdx.x * 128;
  for (int t = tid; t < NB * NB; t += 256) Z[t / NB][t % NB] = Linv[t];
  for (int t = tid; t < 128 * NB; t += 256) {
    const int rr = t / NB, j = t % NB;
    P[rr][j] = (r0 + rr < nrows && j < nb) ? A[(size_t)(r0 + rr) * lda + k0 + j] : 0.0;
  }
  __syncthreads();
  const int wv = tid >> 6, lane = tid & 63;
  const int li = lane & 15, lk = lane >> 4;
  double4_t acc[2][4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[a][q] = (double4_t){0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int kk = 0; kk < NB; kk += 4) {
    const double a0 = P[32 * wv + li][kk + lk];
    const double a1 = P[32 * wv + 16 + li][kk + lk];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double b = Z[16 * q + li][kk + lk];
      acc[0][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, acc[0][q], 0, 0, 0);
      acc[1][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, acc[1][q], 0, 0, 0);
    }
  }
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = r0 + 32 * wv + 16 * a + lk + 4 * reg;
        const int col = 16 * q + li;
        if (row < nrows && col < nb) A[(size_t)row * lda + k0 + col] = acc[a][q][reg];
      }
}

// Trailing update with FP64 MFMA.  Tile = 64 x 64 outputs per workgroup of 256
// threads (4 waves); wave w owns output rows [16w, 16w+16) x 64 columns = four
// 16x16 MFMA accumulators.  C[i][j] -= sum_k P[i][k] * P[j][k], k < nb.
//   v_mfma_f64_16x16x4_f64: A[i=l&15][k=l>>4], B[k=l>>4][j=l&15],
//   C/D: col = l&15, row = (l>>4) + 4*reg   (f64 layout, see CDNA guide sec.3)
__global__ __launch_bounds__(256) void k_syrk(double* __restrict__ A, int lda, int nrows, int k0, int nb,
                                              const int* __restrict__ skip) {
  const int base = k0 + nb;  // first trailing row/col
  const int ti = blockIdx.y, tj = blockIdx.x;
  if (tj > ti || (skip && *skip)) return;  // lower tiles only
  const int r0 = base + ti * 64, c0 = base + tj * 64;
  __shared__ double Pr[64][LDP];  // rows of the panel for this tile's rows
  __shared__ double Pc[64][LDP];  // rows of the panel for this tile's cols
  const int tid = threadIdx.x;
  const int wv = tid >> 6, lane = tid & 63;
  const int li = lane & 15, lk = lane >> 4;
  // prefetch the C tile (independent of the panel loads) to overlap one memory round trip
  double4_t cold[4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = r0 + 16 * wv + lk + 4 * reg;
      const int col = c0 + 16 * q + li;
      const bool ok = row < nrows && col <= row && col < nrows - 1;
      cold[q][reg] = ok ? A[(size_t)row * lda + col] : 0.0;
    }
  for (int t = tid; t < 64 * NB; t += 256) {
    const int i = t / NB, k = t % NB;
    const int rr = r0 + i, cc = c0 + i;
    Pr[i][k] = (rr < nrows && k < nb) ? A[(size_t)rr * lda + k0 + k] : 0.0;
    Pc[i][k] = (cc < nrows && k < nb) ? A[(size_t)cc * lda + k0 + k] : 0.0;
  }
  __syncthreads();
  double4_t acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = (double4_t){0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int kk = 0; kk < NB; kk += 4) {
    const double a = Pr[16 * wv + li][kk + lk];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double b = Pc[16 * q + li][kk + lk];
      acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[q], 0, 0, 0);
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = r0 + 16 * wv + lk + 4 * reg;
      const int col = c0 + 16 * q + li;
      // the rhs row (row == nrows-1) has columns < nrows-1 only
      if (row < nrows && col <= row && col < nrows - 1) A[(size_t)row * lda + col] = cold[q][reg] - acc[q][reg];
    }
}

// Backward substitution x = L^-T y in 64-wide block steps with the block
// inverses saved by k_potrf: x_k = Linv_k^T y_k, then y_j -= L[k-rows][j]^T x_k
// spread over one workgroup per 256 columns.
__device__ __forceinline__ void back_step(const double* __restrict__ A, int lda, int n, int kb,
                                          const double* __restrict__ Linv, double* __restrict__ y,
                                          double* __restrict__ x) {
  __shared__ double yk[NB], xk[NB], part[4][NB];
  const int k0 = kb * NB;
  const int nb = min(NB, n - k0);
  const int tid = threadIdx.x;
  if (tid < NB) yk[tid] = (tid < nb) ? y[k0 + tid] : 0.0;
  __syncthreads();
  {
    // x_k[i] = sum_r Linv[r][i] y_k[r] : 4 row chunks of 16 per column i
    const int i = tid & 63, ch = tid >> 6;
    const double* Z = Linv + (size_t)kb * NB * NB;
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) { const int r = ch * 16 + q; s += Z[r * NB + i] * yk[r]; }
    part[ch][i] = s;
  }
  __syncthreads();
  if (tid < NB) {
    const double s = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
    xk[tid] = s;
    if (blockIdx.x == 0 && tid < nb) x[k0 + tid] = s;
  }
  __syncthreads();
  const int j = blockIdx.x * 256 + tid;
  if (j < k0) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    const double* col = A + (size_t)k0 * lda + j;
    if (nb == NB) {
#pragma unroll
      for (int r = 0; r < NB; r += 4) {
        s0 += col[(size_t)r * lda] * xk[r]; s1 += col[(size_t)(r + 1) * lda] * xk[r + 1];
        s2 += col[(size_t)(r + 2) * lda] * xk[r + 2]; s3 += col[(size_t)(r + 3) * lda] * xk[r + 3];
      }
    } else {
      for (int r = 0; r < nb; ++r) s0 += col[(size_t)r * lda] * xk[r];
    }
    y[j] -= (s0 + s1) + (s2 + s3);
  }
}

__global__ __launch_bounds__(256) void k_back_step(const double* __restrict__ A, int lda, int n, int kb,
                                                   const double* __restrict__ Linv, double* __restrict__ y,
                                                   double* __restrict__ x) {
  back_step(A, lda, n, kb, Linv, y, x);
}

// The same step for k right-hand sides at once: blockIdx.y = vector (y, x of vector v at v * ldy, v * ldx).
// Every vector takes k_back_step's arithmetic in k_back_step's order: k = 1 is bit-identical to it.
// skip (optional): the step returns at once while *skip is non-zero (a device-side stopping test, lud_positions.hip).
__global__ __launch_bounds__(256) void k_back_step_multi(const double* __restrict__ A, int lda, int n, int kb,
                                                         const double* __restrict__ Linv, double* __restrict__ y, int ldy,
                                                         double* __restrict__ x, int ldx, const int* __restrict__ skip) {
  if (skip && *skip) return;
  back_step(A, lda, n, kb, Linv, y + (size_t)blockIdx.y * ldy, x + (size_t)blockIdx.y * ldx);
}

// Forward substitution y = L^-1 b against a stored factor, k vectors (blockIdx.y = vector), one 64-row block step:
//   y_k = Linv_k b_k            (every workgroup forms it; workgroup 0 writes it to y)
//   b_j -= L[j][k-cols] y_k     for the rows j >= k0 + nb, one wavefront per row (lane = column, butterfly sum),
//                               16 rows per workgroup.
// b is read only in block k and written only below it, y is written only in block k: no workgroup reads what
// another one writes in the same launch.
__global__ __launch_bounds__(256) void k_fwd_step_multi(const double* __restrict__ A, int lda, int n, int kb,
                                                        const double* __restrict__ Linv, double* __restrict__ b, int ldb,
                                                        double* __restrict__ y, int ldy, const int* __restrict__ skip) {
  __shared__ double bk[NB], yk[NB], part[4][NB];
  if (skip && *skip) return;
  b += (size_t)blockIdx.y * ldb;
  y += (size_t)blockIdx.y * ldy;
  const int k0 = kb * NB;
  const int nb = min(NB, n - k0);
  const int tid = threadIdx.x;
  if (tid < NB) bk[tid] = (tid < nb) ? b[k0 + tid] : 0.0;
  __syncthreads();
  {
    // y_k[i] = sum_r Linv[i][r] b_k[r] : 4 column chunks of 16 per row i
    const int i = tid & 63, ch = tid >> 6;
    const double* Z = Linv + (size_t)kb * NB * NB;
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) { const int r = ch * 16 + q; s += Z[i * NB + r] * bk[r]; }
    part[ch][i] = s;
  }
  __syncthreads();
  if (tid < NB) {
    const double s = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
    yk[tid] = s;
    if (blockIdx.x == 0 && tid < nb) y[k0 + tid] = s;
  }
  __syncthreads();
  const int lane = tid & 63, wv = tid >> 6;
  const double yl = lane < nb ? yk[lane] : 0.0;
  for (int q = 0; q < 4; ++q) {
    const int j = k0 + nb + blockIdx.x * 16 + wv * 4 + q;   // wave-uniform
    if (j >= n) break;
    const double t = lane < nb ? A[(size_t)j * lda + k0 + lane] * yl : 0.0;
    const double s = wave_sum_butterfly(t);
    if (lane == 0) b[j] -= s;
  }
}

}  // namespace

size_t dense_cholesky_workspace(int n) {
  const int nblk = (n + NB - 1) / NB;
  return (size_t)std::max(1, nblk) * NB * NB + (size_t)n + 8;
}

void dense_cholesky_factor(int n, int k, double* A, int lda, double* work, double* fail_flag, hipStream_t st,
                           const int* skip) {
  if (n <= 0) return;
  const int nrows = n + k;  // rows n .. n+k-1 = right-hand sides, forward-substituted in place
  const int nblk = (n + NB - 1) / NB;
  double* Linv = work;
  for (int kb = 0; kb < nblk; ++kb) {
    const int k0 = kb * NB;
    const int nb = (n - k0 < NB) ? (n - k0) : NB;
    const int below = nrows - (k0 + nb);
    double* Zk = Linv + (size_t)kb * NB * NB;
    k_potrf<<<1, 256, 0, st>>>(A, lda, k0, nb, Zk, fail_flag, skip);
    if (below > 0) {
      k_trsm<<<(below + 127) / 128, 256, 0, st>>>(A, lda, nrows, k0, nb, Zk, skip);
      const int tiles = (below + 63) / 64;
      dim3 grid(tiles, tiles);
      k_syrk<<<grid, 256, 0, st>>>(A, lda, nrows, k0, nb, skip);
    }
  }
}

void dense_cholesky_back_substitute(int n, const double* A, int lda, const double* work, int k, double* Y, int ldy,
                                    double* X, int ldx, hipStream_t st, const int* skip) {
  if (n <= 0 || k <= 0) return;
  const int nblk = (n + NB - 1) / NB;
  for (int kb = nblk - 1; kb >= 0; --kb) {
    const int k0 = kb * NB;
    dim3 grid(k0 > 0 ? (k0 + 255) / 256 : 1, k);
    k_back_step_multi<<<grid, 256, 0, st>>>(A, lda, n, kb, work, Y, ldy, X, ldx, skip);
  }
}

void dense_cholesky_solve_factored(int n, const double* A, int lda, const double* work, int k, double* B, int ldb,
                                   double* T, double* X, int ldx, hipStream_t st, const int* skip) {
  if (n <= 0 || k <= 0) return;
  const int nblk = (n + NB - 1) / NB;
  for (int kb = 0; kb < nblk; ++kb) {
    const int below = n - std::min(n, (kb + 1) * NB);
    dim3 grid(below > 0 ? (below + 15) / 16 : 1, k);
    k_fwd_step_multi<<<grid, 256, 0, st>>>(A, lda, n, kb, work, B, ldb, T, n, skip);
  }
  dense_cholesky_back_substitute(n, A, lda, work, k, T, n, X, ldx, st, skip);
}

void dense_cholesky_solve(int n, double* A, int lda, double* b, double* work, double* fail_flag, hipStream_t st) {
  if (n <= 0) return;
  // row n = right-hand side (b must alias A + n*lda): the factorisation leaves y = L^-1 b there
  dense_cholesky_factor(n, 1, A, lda, work, fail_flag, st, nullptr);
  const int nblk = (n + NB - 1) / NB;
  double* Linv = work;
  double* x = work + (size_t)nblk * NB * NB;
  double* y = A + (size_t)n * lda;
  for (int kb = nblk - 1; kb >= 0; --kb) {
    const int k0 = kb * NB;
    const int grid = k0 > 0 ? (k0 + 255) / 256 : 1;
    k_back_step<<<grid, 256, 0, st>>>(A, lda, n, kb, Linv, y, x);
  }
  (void)hipMemcpyAsync(b, x, sizeof(double) * n, hipMemcpyDeviceToDevice, st);
}

}  // namespace thip

using namespace thip;

// Introspection for the parity tests: factor A once, then solve the k right-hand sides against the factor
// (dense_cholesky_solve_factored: the forward and backward kernels of the ADMM solves).
extern "C" int theia_hip_dense_spd_solve_multi(int32_t n, const double* A, int32_t k, const double* B, double* X) {
  if (n < 0 || k < 1 || (n > 0 && (!A || !B || !X))) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "bad argument");
  if (n == 0) return 0;
  int rc = thip::ensure_device();
  if (rc) return rc;
  DenseSpd S;   // row n: the factorisation's right-hand-side row (zero, unused)
  DevBuf<double> dB, dT, dX;
  if ((rc = S.alloc(n, 1)) || (rc = dB.up(B, (size_t)k * n)) || (rc = dT.alloc((size_t)k * n)) || (rc = dX.alloc((size_t)k * n)))
    return rc;
  if ((rc = S.clear(nullptr, true))) return rc;
  HIP_TRY(hipMemcpy2D(S.A(), sizeof(double) * S.lda, A, sizeof(double) * n, sizeof(double) * n, n, hipMemcpyHostToDevice));
  S.factor(1, nullptr);
  S.solve_factored(k, dB.p, dT.p, dX.p, nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(X, dX.p, sizeof(double) * (size_t)k * n, hipMemcpyDeviceToHost));
  bool failed = false;
  if ((rc = S.failed(&failed))) return rc;
  if (failed) return set_error(THEIA_HIP_ERR_INTERNAL, "matrix is not positive definite");
  return 0;
}
