// smallest_eigenvector.h -- what the two position stages share that take the camera positions as the eigenvector of the
// smallest eigenvalue of normal equations summed on 3 x 3 view blocks (ligt_positions.hip, linear_positions.hip): the
// owner sums that assemble the lower triangle from per-constraint 3 x 3 items without atomics, the host plan that lists
// every block's items, the one-vector inverse iteration step with its stopping test on the device, and the view pairs'
// sign vote.  spectral_shift.h has the shift that goes in front of the factorisation.  SmallestEigenvector, at the end,
// is the host driver of all of it: what used to be the last 120 lines of each of the two entry points.
//
// Determinism: every entry of H is a sum in the order of the plan by one owner, every norm a fixed tree (block_sum), the
// votes are integers.
#ifndef THEIA_HIP_SMALLEST_EIGENVECTOR_H_
#define THEIA_HIP_SMALLEST_EIGENVECTOR_H_
#include "small_linalg.h"
#include "rotation_maps.h"
#include "dense_cholesky.h"
#include "spectral_shift.h"
#include "wave_reduce.h"

#include <algorithm>
#include <chrono>
#include <vector>

namespace thip {

struct InverseIterationState {
  int done, converged, iterations, pad;
  double diff, eigenvalue, shift, max_diag;
};

using rsc::cross3;

// out = X' Y (3 x 3, row-major)
__device__ __forceinline__ void atb(const double* X, const double* Y, double* out) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * r + c] = (X[r] * Y[c] + X[3 + r] * Y[3 + c]) + X[6 + r] * Y[6 + c];
}

__device__ __forceinline__ void store9(double* __restrict__ dst, const double* v) {
#pragma unroll
  for (int k = 0; k < 9; ++k) dst[k] = v[k];
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_rotations(int n, const double* __restrict__ aa, double* __restrict__ R) {
  const int v = blockIdx.x * THREADS + threadIdx.x;
  if (v >= n) return;
  double r[9];
  rsc::angle_axis_to_rot(aa + 3 * (size_t)v, r);
#pragma unroll
  for (int k = 0; k < 9; ++k) R[9 * (size_t)v + k] = r[k];
}

// The items of every non-empty 3 x 3 block of the lower triangle (row >= col, free views), in the order the stage
// visits them.  seg_item = item index * 2 + (1: the item is added transposed).
struct BlockSegments {
  std::vector<int2> block_rc;
  std::vector<long long> seg_off;
  std::vector<int> seg_item;
};

// visit(emit) calls emit(a, b, item) for every item X' Y with X on the view of index a and Y on the view of index b, in
// the order of summation; an index < 0 is the held view and the item is left out.  The item lands on block (a, b),
// transposed when that lies above the diagonal.  A stable counting sort by block over mf free views.
template <class Visit>
inline void build_block_segments(int mf, Visit&& visit, BlockSegments* out) {
  const size_t tri = (size_t)mf * (mf + 1) / 2;
  std::vector<long long> seg_start(tri + 1, 0);
  auto block_of = [](int a, int b) { return a >= b ? (size_t)a * (a + 1) / 2 + b : (size_t)b * (b + 1) / 2 + a; };
  visit([&](int a, int b, long long) { if (a >= 0 && b >= 0) seg_start[block_of(a, b) + 1] += 1; });
  for (size_t k = 0; k < tri; ++k) seg_start[k + 1] += seg_start[k];
  out->seg_item.assign((size_t)std::max<long long>(1, seg_start[tri]), 0);
  {
    std::vector<long long> fill(seg_start.begin(), seg_start.end() - 1);
    visit([&](int a, int b, long long it) {
      if (a >= 0 && b >= 0) out->seg_item[(size_t)fill[block_of(a, b)]++] = (int)(2 * it + (a < b ? 1 : 0));
    });
  }
  out->block_rc.clear();
  out->seg_off.assign(1, 0);
  for (int a = 0; a < mf; ++a)
    for (int b = 0; b <= a; ++b) {
      const size_t k = block_of(a, b);
      if (seg_start[k + 1] > seg_start[k]) { out->block_rc.push_back(make_int2(a, b)); out->seg_off.push_back(seg_start[k + 1]); }
    }
}

// One thread per non-empty block of H's lower triangle: its items in the plan's order.  A diagonal block writes its own
// lower triangle only.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_blocks(int num_blocks, const int2* __restrict__ block_rc,
                                                    const long long* __restrict__ seg_off, const int* __restrict__ seg_item,
                                                    const double* __restrict__ items, int lda, double* __restrict__ H) {
  const int b = blockIdx.x * THREADS + threadIdx.x;
  if (b >= num_blocks) return;
  double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (long long k = seg_off[b]; k < seg_off[b + 1]; ++k) {
    const int it = seg_item[k];
    const double* v = items + 9 * (size_t)(it >> 1);
    if (it & 1) {
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[3 * r + c] += v[3 * c + r];
    } else {
#pragma unroll
      for (int q = 0; q < 9; ++q) acc[q] += v[q];
    }
  }
  const int2 rc = block_rc[b];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if (rc.x != rc.y || c <= r) H[(size_t)(3 * rc.x + r) * lda + 3 * rc.y + c] = acc[3 * r + c];
}

// system_out: both triangles of the n x n system from the lower triangle (before the shift)
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_full_system(int n, int lda, const double* __restrict__ H,
                                                         double* __restrict__ full) {
  const size_t k = (size_t)blockIdx.x * THREADS + threadIdx.x;
  if (k >= (size_t)n * n) return;
  const int r = (int)(k / n), c = (int)(k % n);
  full[k] = r >= c ? H[(size_t)r * lda + c] : H[(size_t)c * lda + r];
}

// One workgroup, after y = (H + mu I)^-1 x: x_new = y / |y|, the step |x_new - s x|_2 with s = sign(x_new . x), the
// Rayleigh quotient of y as the eigenvalue estimate, the iteration count and the stop flag.  b = x_new for the next solve.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_iterate(int n, const double* __restrict__ y, double* __restrict__ x,
                                                     double* __restrict__ b, double threshold,
                                                     InverseIterationState* __restrict__ st) {
  __shared__ double red[THREADS];
  if (st->done) return;
  double yy = 0.0, yx = 0.0;
  for (int k = threadIdx.x; k < n; k += THREADS) { yy += y[k] * y[k]; yx += y[k] * x[k]; }
  const double syy = block_sum<THREADS>(yy, red), syx = block_sum<THREADS>(yx, red);
  __shared__ double bc[2];
  if (threadIdx.x == 0) { bc[0] = sqrt(syy); bc[1] = syx; }
  __syncthreads();
  const double norm = bc[0], dot = bc[1];
  if (!(norm > 0.0) || !isfinite(norm)) {   // a breakdown of the solve: stop, not converged, x stays
    if (threadIdx.x == 0) { st->iterations += 1; st->done = 1; st->converged = 0; st->diff = norm; }
    return;
  }
  const double s = dot < 0.0 ? -1.0 : 1.0;
  double dd = 0.0;
  for (int k = threadIdx.x; k < n; k += THREADS) {
    const double xn = y[k] / norm, d = xn - s * x[k];
    dd += d * d;
    x[k] = xn; b[k] = xn;
  }
  const double sdd = block_sum<THREADS>(dd, red);
  if (threadIdx.x == 0) {
    const double diff = sqrt(sdd);
    st->iterations += 1;
    st->diff = diff;
    st->eigenvalue = dot / syy - st->shift;
    if (diff <= threshold) { st->done = 1; st->converged = 1; }
  }
}

// VectorsAreSameDirection per view pair whose two views are in the system: +1 when
// (R_first (c_second - c_first) / |.|) . position_2 > 0, else -1.  idx: -1 held (the origin), -2 not in the system.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_sign_vote(int E, const int2* __restrict__ edges, const int* __restrict__ idx,
                                                       const double* __restrict__ x, const double* __restrict__ R,
                                                       const double* __restrict__ rel, int* __restrict__ votes) {
  __shared__ int red[THREADS];
  const int e = blockIdx.x * THREADS + threadIdx.x;
  int vote = 0;
  if (e < E) {
    const int2 ij = edges[e];
    const int a = idx[ij.x], c = idx[ij.y];
    if (a != -2 && c != -2) {
      double d[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) d[k] = (c >= 0 ? x[3 * (size_t)c + k] : 0.0) - (a >= 0 ? x[3 * (size_t)a + k] : 0.0);
      const double nrm = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
      if (nrm > 0.0) { d[0] /= nrm; d[1] /= nrm; d[2] /= nrm; }
      const double* r = R + 9 * (size_t)ij.x;
      double dot = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) dot += ((r[3 * k] * d[0] + r[3 * k + 1] * d[1]) + r[3 * k + 2] * d[2]) * rel[3 * (size_t)e + k];
      vote = dot > 0.0 ? 1 : -1;
    }
  }
  red[threadIdx.x] = vote;
  __syncthreads();
  for (int s = THREADS / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0 && red[0] != 0) atomicAdd(votes, red[0]);
}

// The host side after a stage has its view index and its items' plan: H + mu I from a device array of 3 x 3 items, one
// factorisation, the inverse iteration in chunks, the sign vote, the scatter.  The steps are called in the order they
// are declared; what the two stages do differently (their items kernel, the *_ms field a phase is booked to, whether
// there are view pairs to vote) stays between the calls.  Summary: theia_ligt_summary or theia_linear_triplet_summary.
struct SmallestEigenvector {
  static constexpr int kThreads = 256;
  static constexpr int kChunk = 4;   // inverse iterations enqueued between two reads of the `done` flag
  int n3 = 0, num_blocks = 0;
  DenseSpd H;   // row n3: the factorisation's right-hand-side row (zero, unused)
  DevBuf<double> d_full, d_x, d_b, d_y, d_T;
  DevBuf<long long> d_seg_off;
  DevBuf<int> d_seg_item, d_votes;
  DevBuf<int2> d_block_rc;
  DevBuf<InverseIterationState> d_st;
  InverseIterationState hs{};
  int votes = 0;
  std::vector<double> x, full;

  // The dense system of mf free views first: when it does not fit, that is the answer, before the host builds lists of
  // its size.  want_full: system_out is asked for.
  int alloc(int mf, bool want_full) {
    n3 = 3 * mf;
    int rc;
    if ((rc = H.alloc(n3, 1)) || (want_full && (rc = d_full.alloc((size_t)n3 * n3)))) return rc;
    return 0;
  }
  // the plan, the vectors, and everything cleared (enqueued, not waited for)
  int upload(const BlockSegments& seg, hipStream_t st) {
    num_blocks = (int)seg.block_rc.size();
    int rc;
    if ((rc = d_seg_off.up(seg.seg_off.data(), seg.seg_off.size())) || (rc = d_seg_item.up(seg.seg_item.data(), seg.seg_item.size())) ||
        (rc = d_block_rc.up(seg.block_rc.data(), seg.block_rc.size())) || (rc = d_votes.alloc(1)) || (rc = d_x.alloc(n3)) ||
        (rc = d_b.alloc(n3)) || (rc = d_y.alloc(n3)) || (rc = d_T.alloc(n3)) || (rc = d_st.alloc(1)) || (rc = H.clear(st, true)))
      return rc;
    HIP_TRY(hipMemsetAsync(d_votes.p, 0, sizeof(int), st));
    HIP_TRY(hipMemsetAsync(d_st.p, 0, sizeof(InverseIterationState), st));
    return 0;
  }
  // H from the items, system_out's copy of it, the shift and the start vector; waits for them
  int assemble(const double* d_items, double shift_multiple, hipStream_t st) {
    k_blocks<kThreads><<<grid_of(num_blocks, kThreads), kThreads, 0, st>>>(num_blocks, d_block_rc.p, d_seg_off.p, d_seg_item.p,
                                                                          d_items, H.lda, H.A());
    if (d_full.p)
      k_full_system<kThreads><<<grid_of((size_t)n3 * n3, kThreads), kThreads, 0, st>>>(n3, H.lda, H.A(), d_full.p);
    k_shift<kThreads><<<1, kThreads, 0, st>>>(n3, H.lda, H.A(), shift_multiple, d_x.p, d_b.p, &d_st.p->shift, &d_st.p->max_diag);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
  }
  // factors H + mu I once; a failure leaves *out = *sm with the shift and is the error returned
  template <class Summary>
  int factor(hipStream_t st, Summary* sm, Summary* out) {
    const auto t_factor = std::chrono::steady_clock::now();
    H.factor(1, st);
    bool failed = false;
    if (int rc = H.failed(&failed)) return rc;
    sm->factor_ms = ms_since(t_factor);
    if (failed) {
      HIP_TRY(hipMemcpy(&hs, d_st.p, sizeof(InverseIterationState), hipMemcpyDeviceToHost));
      sm->shift = hs.shift;
      *out = *sm;
      return set_error(THEIA_HIP_ERR_INTERNAL, "the Cholesky factorisation of H + mu I failed (mu = %g)", hs.shift);
    }
    return 0;
  }
  // inverse iteration from x = 1 / sqrt(n) until the step is <= threshold or the cap
  int iterate(int max_iterations, double threshold, hipStream_t st) {
    const int* done = &d_st.p->done;
    return run_until_done(max_iterations, kChunk, d_st.p, &hs, [&]() {
      H.solve_factored(1, d_b.p, d_T.p, d_y.p, st, done);
      k_iterate<kThreads><<<1, kThreads, 0, st>>>(n3, d_y.p, d_x.p, d_b.p, threshold, d_st.p);
      return 0;
    });
  }
  int vote(int E, const int2* edges, const int* idx, const double* R, const double* rel, hipStream_t st) {
    k_sign_vote<kThreads><<<grid_of(E, kThreads), kThreads, 0, st>>>(E, edges, idx, d_x.p, R, rel, d_votes.p);
    HIP_TRY(hipGetLastError());
    return 0;
  }
  int fetch() {
    x.resize(n3);
    HIP_TRY(hipMemcpy(x.data(), d_x.p, sizeof(double) * (size_t)n3, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&votes, d_votes.p, sizeof(int), hipMemcpyDeviceToHost));
    if (d_full.p) {
      full.resize((size_t)n3 * n3);
      HIP_TRY(hipMemcpy(full.data(), d_full.p, sizeof(double) * full.size(), hipMemcpyDeviceToHost));
    }
    return 0;
  }
  // idx [n]: >= 0 the view's index in the system, -1 the held view (the origin), -2 not in the system
  template <class Summary>
  void scatter(int n, const std::vector<int>& idx, double* positions_out, uint8_t* estimated_out, double* system_out,
               int32_t* system_index_out, Summary* sm) const {
    sm->iterations = hs.iterations;
    sm->converged = hs.converged;
    sm->eigenvalue = hs.eigenvalue;
    sm->shift = hs.shift;
    sm->sign_votes = votes;
    sm->flipped = votes < 0;
    const double sign = votes < 0 ? -1.0 : 1.0;
    for (int v = 0; v < n; ++v) {
      estimated_out[v] = idx[v] != -2;
      if (idx[v] == -2) continue;
      for (int c = 0; c < 3; ++c) positions_out[3 * (size_t)v + c] = idx[v] >= 0 ? sign * x[3 * (size_t)idx[v] + c] : 0.0;
    }
    if (system_out) std::copy(full.begin(), full.end(), system_out);
    if (system_index_out) std::copy(idx.begin(), idx.end(), system_index_out);
  }
};

}  // namespace thip
#endif
