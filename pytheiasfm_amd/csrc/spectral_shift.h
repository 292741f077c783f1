// spectral_shift.h -- the diagonal shift of the stages that take eigenvectors of the smallest eigenvalues by inverse
// iteration over one dense Cholesky (ligt_positions.hip, linear_positions.hip, linear_rotations.hip).  On noise-free input those eigenvalues
// are rounding errors of either sign, so the matrix itself may have no Cholesky factor; H + mu I with
//   mu = multiple n eps max diag H
// has one, and the shift moves no eigenvector (DESIGN.md 3.6f has the rule and the scenes it was chosen on).
#ifndef THEIA_HIP_SPECTRAL_SHIFT_H_
#define THEIA_HIP_SPECTRAL_SHIFT_H_
#include <hip/hip_runtime.h>

#include <cfloat>

namespace thip {

// One workgroup of THREADS: max diag H over the n rows, then mu on the diagonal.  x and b (both or neither): the start
// vector 1 / sqrt(n) of a one-vector iteration.  *shift_out = mu, *max_diag_out = max diag H before the shift.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_shift(int n, int lda, double* __restrict__ H, double multiple,
                                                   double* __restrict__ x, double* __restrict__ b,
                                                   double* __restrict__ shift_out, double* __restrict__ max_diag_out) {
  __shared__ double red[THREADS];
  double m = 0.0;
  for (int k = threadIdx.x; k < n; k += THREADS) m = fmax(m, H[(size_t)k * lda + k]);
  red[threadIdx.x] = m;
  __syncthreads();
  for (int s = THREADS / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  const double max_diag = red[0];
  const double mu = ((multiple * (double)n) * DBL_EPSILON) * max_diag;
  const double x0 = 1.0 / sqrt((double)n);
  for (int k = threadIdx.x; k < n; k += THREADS) {
    H[(size_t)k * lda + k] += mu;
    if (x) { x[k] = x0; b[k] = x0; }
  }
  if (threadIdx.x == 0) { *shift_out = mu; *max_diag_out = max_diag; }
}

}  // namespace thip
#endif
